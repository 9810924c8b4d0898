"""CPU: the one end of every backward launcher, ``dense._finish_partials`` -- the section tables of the partial rows, which sections
are queued inside ``deferred_param_grads()`` and which reducer finishes the rest -- and the node-side predicate
``dense._queue_params``.  No kernel runs: the three reducers are stand-ins that record their calls, ``_deferrable`` is a switch.
Which buffers a real step queues: tests/test_gpu_deferred_census.py; that queued and eager gradients agree bitwise:
tests/test_gpu_deferred.py."""
import math
from types import SimpleNamespace

import pytest
import torch

from allset_amd import _lib, dense

O, I, D = 8, 12, 8
PARAM_KEYS = ("weight", "bias", "gamma", "beta", "colb")        # (the auxiliary rows belong to a folded tensor, never to a parameter)


def _tables():
    out = {}
    for colb in (None, (D,), (1, 2, D // 2)):
        out[f"ln colb={colb}"] = dense._ln_sections(D, colb)
    for bias in (True, False):
        for aux in (False, True):
            out[f"wgrad bias={bias} aux={aux}"] = dense._wgrad_sections(O, I, bias, aux=aux)
            out[f"one-pass bias={bias} aux={aux}"] = dense._one_pass_sections(O, I, bias, aux=aux)           # bwd_all / _aux / narrow
        for ln in (I, O):                                                                                    # bwd_all, ln_pro
            out[f"one-pass bias={bias} ln={ln}"] = dense._one_pass_sections(O, I, bias, ln=ln)
        for colb in ((I,), (1, 3, I // 3)):                                                                  # pma_tail
            out[f"one-pass bias={bias} ln colb={colb}"] = dense._one_pass_sections(O, I, bias, ln=I, colb_shape=colb)
    out["hop epilogue"] = [("bias", 0, (D,))]
    return out


TABLES = _tables()


def _width(sections):
    return (max(off + math.prod(shape) for _, off, shape in sections) + 3) // 4 * 4          # (the launchers pad the row to 4 floats)


def _part(sections, rows=3):
    return torch.arange(_width(sections), dtype=torch.float32).repeat(rows, 1)


def _params(sections):
    return {k: torch.nn.Parameter(torch.zeros(shape)) for k, _, shape in sections if k in PARAM_KEYS}


@pytest.fixture
def calls(monkeypatch):
    """The three reducers as sums that record ``(name, args)``; ``calls.deferrable`` answers ``_deferrable``."""
    log = SimpleNamespace(made=[], deferrable=True, asked=[])

    def whole(part):
        log.made.append(("reduce_partials", tuple(part.shape)))
        return part.sum(0)

    def to(part, M, dtype):
        log.made.append(("reduce_partials_to", tuple(part.shape), M, dtype))
        return part[:, :M].sum(0).to(dtype)

    def slice_(part, col0, M, dtype):
        log.made.append(("reduce_partials_slice", tuple(part.shape), col0, M, dtype))
        return part[:, col0:col0 + M].sum(0).to(dtype)

    def deferrable(part, *params, M=None):
        log.asked.append((tuple(part.shape), params, M))
        return log.deferrable

    monkeypatch.setattr(dense, "reduce_partials", whole)
    monkeypatch.setattr(dense, "reduce_partials_to", to)
    monkeypatch.setattr(dense, "reduce_partials_slice", slice_)
    monkeypatch.setattr(dense, "_deferrable", deferrable)
    return log


@pytest.fixture
def scope():
    """Inside ``deferred_param_grads()``; left without a flush (there is no device to reduce on), the queue cleared by hand."""
    s = dense.deferred_param_grads()
    s.__enter__()
    yield dense._Deferred
    dense._Deferred.active, dense._Deferred.pending = False, []


def _assert_views(sections, grads, rows=3, base=0):
    assert len(grads) == len(sections)
    for (key, off, shape), g in zip(sections, grads):
        n = math.prod(shape)
        assert tuple(g.shape) == tuple(shape), key
        assert torch.equal(g.reshape(-1), (rows * torch.arange(off, off + n, dtype=torch.float32)).to(g.dtype)), key       # (bf16: rounded once)


@pytest.mark.parametrize("name", list(TABLES))
def test_sections_are_disjoint_and_the_views_are_their_columns(name, calls):
    sections = TABLES[name]
    spans = sorted((off, off + math.prod(shape)) for _, off, shape in sections)
    assert spans[0][0] >= 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= _width(sections)
    assert len({k for k, _, _ in sections}) == len(sections)
    part = _part(sections)
    _assert_views(sections, dense._finish_partials(part, sections))
    assert calls.made == [("reduce_partials", tuple(part.shape))] and not calls.asked         # fp32, the full row: the plain reducer
    # outside the scope the real _deferrable says no; here the switch does: parameters given, nothing queueable -> the same one launch
    calls.deferrable, calls.made = False, []
    _assert_views(sections, dense._finish_partials(part, sections, _params(sections)))
    assert calls.made == [("reduce_partials", tuple(part.shape))] and not dense._Deferred.pending


def test_a_three_axis_buffer_is_flattened_and_bf16_is_rounded_by_the_reduction(calls):
    sections = dense._ln_sections(D, (D,))
    part = _part(sections).view(3, 3, D)
    _assert_views(sections, dense._finish_partials(part, sections))
    assert calls.made == [("reduce_partials", (3, 3 * D))]
    calls.made = []
    grads = dense._finish_partials(part, sections, out_dtype=torch.bfloat16)
    assert calls.made == [("reduce_partials_to", (3, 3 * D), 3 * D, torch.bfloat16)] and all(g.dtype == torch.bfloat16 for g in grads)
    # the bf16 kernel takes rows of a multiple of 4 floats and at most 4096 of them: otherwise the fp32 sum, cast
    for odd in (torch.zeros(3, 3, 6), torch.zeros(4097, 3 * D)):
        calls.made = []
        secs = dense._ln_sections(odd[0].numel() // 3, (odd[0].numel() // 3,))
        grads = dense._finish_partials(odd, secs, out_dtype=torch.bfloat16)
        assert calls.made == [("reduce_partials", (odd.shape[0], odd[0].numel()))] and all(g.dtype == torch.bfloat16 for g in grads)
    # a row narrower than its stride (a column slice of a wider buffer) cannot go through the plain reducer
    calls.made = []
    wide = torch.arange(40, dtype=torch.float32).repeat(3, 1)[:, :3 * D]
    _assert_views(sections, dense._finish_partials(wide, sections))
    assert calls.made == [("reduce_partials_to", (3, 3 * D), 3 * D, torch.float32)]


@pytest.mark.parametrize("name", list(TABLES))
def test_parameter_sections_are_queued_and_the_rest_keeps_the_buffers_association(name, calls, scope):
    sections = TABLES[name]
    part, params = _part(sections), _params(sections)
    own = [s for s in sections if s[0] in params]
    rest = [s for s in sections if s[0] not in params]
    M_main = rest[0][1] if rest else part.shape[1]
    for dtype in (torch.float32, torch.bfloat16):
        calls.made, calls.asked, scope.pending = [], [], []
        grads = dense._finish_partials(part, sections, params, out_dtype=dtype)
        assert grads[:len(own)] == [None] * len(own)
        assert len(scope.pending) == 1
        q_part, q_M, q_secs = scope.pending[0]
        assert q_part.data_ptr() == part.data_ptr() and q_M == M_main
        assert len(q_secs) == len(own) and all(qp is params[k] and (qo, qs) == (off, shape)
                                               for (qp, qo, qs), (k, off, shape) in zip(q_secs, own))
        assert [a[2] for a in calls.asked] == [M_main] and set(map(id, calls.asked[0][1])) == set(map(id, params.values()))
        if rest:
            width = rest[-1][1] + math.prod(rest[-1][2]) - M_main
            assert calls.made == [("reduce_partials_slice", tuple(part.shape), M_main, width, dtype)]
            _assert_views(rest, grads[len(own):])
            assert all(g.dtype == dtype for g in grads[len(own):])
        else:
            assert calls.made == []


@pytest.mark.parametrize("name", list(TABLES))
def test_the_kept_exceptions_still_reduce_the_whole_buffer_at_once(name, calls, scope):
    """DESIGN.md lists the call sites that today do not queue although the rule could: each passes ``queue=False`` or no
    parameters, and then nothing is asked, nothing queued and ONE whole-buffer reduction runs."""
    sections = TABLES[name]
    part, params = _part(sections), _params(sections)
    for kw in (dict(params=params, queue=False), dict(params=None), dict(params={}), dict(params={k: None for k in params})):
        calls.made, calls.asked = [], []
        _assert_views(sections, dense._finish_partials(part, sections, **kw))
        assert calls.made == [("reduce_partials", tuple(part.shape))] and not calls.asked and not scope.pending
    calls.made = []
    dense._finish_partials(part, sections, params, out_dtype=torch.bfloat16, queue=False)
    assert calls.made == [("reduce_partials_to", tuple(part.shape), part.shape[1], torch.bfloat16)] and not scope.pending


def test_the_residual_layer_norm_queues_in_fp32_only_and_a_colb_parameter_keeps_its_shape(calls, scope):
    part = torch.arange(3 * D, dtype=torch.float32).repeat(3, 1).view(3, 3, D)
    colb = torch.zeros(D)
    prm = {"gamma": torch.nn.Parameter(torch.zeros(D)), "beta": torch.nn.Parameter(torch.zeros(D)),
           "colb": torch.nn.Parameter(torch.zeros(1, 2, D // 2))}
    assert dense._finish_ln_res(part, D, colb, prm, torch.float32) == (None, None, None)
    assert [(M, [(o, s) for _, o, s in secs]) for _, M, secs in scope.pending] == [(3 * D, [(0, (D,)), (D, (D,)), (2 * D, (1, 2, D // 2))])]
    # without a colb the node wants two gradients and the WHOLE buffer is queued: no reduction of the third row at once
    scope.pending, calls.made = [], []
    two = {k: prm[k] for k in ("gamma", "beta")}
    assert dense._finish_ln_res(part, D, None, two, torch.float32) == (None, None, None)
    assert [(M, len(secs)) for _, M, secs in scope.pending] == [(3 * D, 2)] and calls.made == []
    # bf16 reduces at once, summed and rounded in one launch (kept)
    scope.pending = []
    dg, db, dc = dense._finish_ln_res(part, D, colb, prm, torch.bfloat16)
    assert calls.made == [("reduce_partials_to", (3, 3 * D), 3 * D, torch.bfloat16)] and not scope.pending
    assert dg.shape == db.shape == (D,) and dc.shape == (1, 2, D // 2)
    # a caller outside a node (no parameters) reads the third row without a colb too
    calls.made = []
    dg, db, dc = dense._finish_ln_res(part, D, None, None, torch.float32)
    assert torch.equal(dc, 3 * torch.arange(2 * D, 3 * D, dtype=torch.float32))


def _ctx(params, need):
    return SimpleNamespace(params=params, needs_input_grad=tuple(need))


def test_the_node_side_predicate(scope):
    w, b = torch.nn.Parameter(torch.zeros(O, I)), torch.nn.Parameter(torch.zeros(O))
    index = {"weight": 1, "bias": 2}
    ctx = _ctx({"weight": w, "bias": b}, (True, True, True))
    got = dense._queue_params(ctx, index)
    assert got == {"weight": w, "bias": b} and got["weight"] is w and got["bias"] is b
    assert set(got) <= {k for k, _, _ in dense._wgrad_sections(O, I)} and set(got) <= {k for k, _, _ in dense._one_pass_sections(O, I)}
    assert dense._queue_params(_ctx({"weight": w, "bias": b}, (True, True, False)), index) is None       # a present parameter does not want its gradient
    assert dense._queue_params(_ctx({"weight": w, "bias": b}, (True, False, True)), index) is None
    got = dense._queue_params(_ctx({"weight": w, "bias": None}, (True, True, False)), index)              # an absent one is ignored ...
    assert list(got) == ["weight"] and got["weight"] is w                                                 # ... and not handed on
    # a node with two buffers asks once per buffer: only the parameters named are looked at
    g, bt = torch.nn.Parameter(torch.zeros(I)), torch.nn.Parameter(torch.zeros(I))
    ctx = _ctx({"gamma": g, "beta": bt, "weight": w, "bias": b}, (True, True, False, True, True))
    assert dense._queue_params(ctx, {"gamma": 1, "beta": 2}) is None
    assert list(dense._queue_params(ctx, {"weight": 3, "bias": 4})) == ["weight", "bias"]
    assert dense._queue_params(SimpleNamespace(needs_input_grad=(True,) * 3), index) is None              # a node that kept no parameters
    scope.active = False
    assert dense._queue_params(_ctx({"weight": w, "bias": b}, (True, True, True)), index) is None         # outside the scope


def test_every_node_keeps_its_parameters_by_key():
    """A node that still kept a tuple would fail only when its backward runs inside the scope: read the sources instead."""
    import ast
    import inspect
    from allset_amd import functional
    found = 0
    for mod in (dense, functional):
        for node in ast.walk(ast.parse(inspect.getsource(mod))):
            if isinstance(node, ast.Assign) and any(isinstance(t, ast.Attribute) and t.attr == "params" and isinstance(t.value, ast.Name)
                                                    and t.value.id == "ctx" for t in node.targets):
                found += 1
                v = node.value
                assert isinstance(v, ast.Dict) or (isinstance(v, ast.Call) and getattr(v.func, "id", None) == "dict"), (mod.__name__, node.lineno)
    assert found >= 12


def test_the_tail_nodes_name_their_parameters_for_both_kernels(scope):
    names = ("att_r", "g0", "b0", "w1", "b1", "w2", "b2", "g1", "bt1")
    import inspect
    from allset_amd import functional
    for node, index in ((dense._PmaTail, dense._TAIL_INPUTS), (functional._PmaPoolTail, functional._POOL_TAIL_INPUTS)):
        args = list(inspect.signature(node.forward).parameters)[1:]                     # (without ctx)
        assert index == {k: args.index(k) for k in names}
    prm = {k: torch.nn.Parameter(torch.zeros(1)) for k in names}
    prm["b1"] = None
    got = dense._queue_params(_ctx(prm, (True,) * 11), dense._TAIL_INPUTS)
    q0 = dense._pick(got, weight="w1", bias="b1", gamma="g0", beta="b0", colb="att_r")
    assert q0["weight"] is prm["w1"] and "bias" not in q0 and q0["gamma"] is prm["g0"] and q0["beta"] is prm["b0"] and q0["colb"] is prm["att_r"]
    assert set(q0) <= {k for k, _, _ in dense._one_pass_sections(O, I, False, ln=I, colb_shape=(I,))}
    assert dense._pick(None, weight="w1") is None


def test_a_parameter_without_a_section_is_refused(calls, scope):
    """What used to be a silently permuted tuple: a key the row does not have."""
    sections = dense._wgrad_sections(O, I, want_bias=False)
    part = _part(sections)
    w, b = torch.nn.Parameter(torch.zeros(O, I)), torch.nn.Parameter(torch.zeros(O))
    for bad in ({"weight": w, "bias": b}, {"weight": w, "wieght": w}, {"gamma": b}):
        for queue in (True, False):
            with pytest.raises(_lib.AllSetHipError, match="section"):
                dense._finish_partials(part, sections, bad, queue=queue)
    assert not scope.pending and not calls.made
    # parameter sections lead the row: a parameter BEHIND a section nobody owns is refused the same way
    with pytest.raises(_lib.AllSetHipError, match="leading sections"):
        dense._finish_partials(_part(dense._wgrad_sections(O, I)), dense._wgrad_sections(O, I), {"bias": b})
