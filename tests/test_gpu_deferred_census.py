"""WHICH partial buffers a backward pass queues inside ``dense.deferred_param_grads()`` and which reducer finishes the rest.  The
bitwise tests (tests/test_gpu_deferred.py, test_gpu_dense.py, test_gpu_random_shapes.py) cannot see this: a buffer that wrongly
reduces at once gives the same bits with one launch more, and the launch sequence of a captured step changes with it.

One forward and backward per case at n = 600 rows and 2,400 incidences: the decision depends on the buffer's (P, M) and on the
parameters, not on the workload's size, and 600 rows give every kernel family more than one partial row.  The expected table below
was printed by this very file on commit e01063e, BEFORE the launchers got their one finishing function (``dense._finish_partials``):
it touches only names both sides have -- ``deferred_param_grads``, ``flush_param_grads``, ``_Deferred.pending`` and the three reducers."""
import pytest
import torch

pytestmark = pytest.mark.gpu

N, DEG = 600, 4


def _grads(params):
    return {k: (p.grad.clone() if p.grad is not None else None) for k, p in params.items()}


def _mlp(width, device):
    from allset_amd import MLP
    torch.manual_seed(3)
    m = MLP(width, width, width, 3, dropout=0.5, Normalization="ln", InputNorm=True).to(device).train()
    x = torch.randn(N, width, device=device)
    G = torch.randn(N, width, device=device)
    return dict(m.named_parameters()), lambda: m(x.clone().requires_grad_(True)).backward(G)


def _pair(model, d, heads, dtype, device):
    from allset_amd import HalfNLHconv, synthetic
    from allset_amd import dist as adist
    torch.manual_seed(21)
    a, b = (HalfNLHconv(d, d, d, 2, 0.5, "ln", True, heads=heads, attention=model == "pma").to(device).to(dtype).train() for _ in range(2))
    hg = synthetic.random_hypergraph(N, N, DEG, seed=9, device=device)
    assert hg.edge_index.shape[1] == N * DEG
    sh = adist.ShardedHypergraph(hg.edge_index, N, N, 1, 0).build_incidences()
    x = torch.randn(N, d, device=device).to(dtype)
    G = torch.randn(N, d, device=device).to(dtype)
    fn, kw = (adist.sharded_pma_layer, {}) if model == "pma" else (adist.sharded_deepsets_layer, {"aggr": "add"})
    params = {f"{s}.{k}": p for s, mod in (("a", a), ("b", b)) for k, p in mod.named_parameters()}
    return params, lambda: fn(a, b, x.clone().requires_grad_(True), sh, dropout=0.5, training=True, **kw).backward(G)


def _linear(bias, device):
    from allset_amd import dense
    torch.manual_seed(4)
    w = torch.nn.Parameter(torch.randn(7, 128, device=device) / 11)
    b = torch.nn.Parameter(torch.randn(7, device=device)) if bias else None
    x = torch.randn(N, 128, device=device)
    G = torch.randn(N, 7, device=device)
    params = {"weight": w, **({"bias": b} if bias else {})}
    return params, lambda: dense.linear(x.clone().requires_grad_(True), w, b).backward(G)


def _project_without_value_bias(device):
    from allset_amd import dense
    torch.manual_seed(5)
    w_v = torch.nn.Parameter(torch.randn(128, 128, device=device) / 11)
    w_a = torch.nn.Parameter(torch.randn(4, 128, device=device) / 11)
    b_a = torch.nn.Parameter(torch.randn(4, device=device))
    x = torch.randn(N, 128, device=device)
    Gv, Ga = torch.randn(N, 128, device=device), torch.randn(N, 4, device=device)

    def run():
        x_v, alpha = dense.pma_project(x.clone().requires_grad_(True), w_v, None, w_a, b_a)
        torch.autograd.backward([x_v, alpha], [Gv, Ga])
    return {"w_v": w_v, "w_a": w_a, "b_a": b_a}, run


def _hconv(device):
    from allset_amd import synthetic
    from allset_amd.baselines import HypergraphConv
    torch.manual_seed(6)
    conv = HypergraphConv(128, 128, bias=True).to(device).train()
    with torch.no_grad():
        conv.bias.normal_()
    hg = synthetic.random_hypergraph(N, N, DEG, seed=9, device=device)
    x = torch.randn(N, 128, device=device)
    G = torch.randn(N, 128, device=device)
    return dict(conv.named_parameters()), lambda: conv(x.clone().requires_grad_(True), hg.edge_index, act="relu", p=0.5).backward(G)


CASES = {
    "mlp64": lambda dev: _mlp(64, dev),
    "mlp128": lambda dev: _mlp(128, dev),
    "mlp256": lambda dev: _mlp(256, dev),                    # the wide path: (weight, bias) and (gamma, beta) decide separately
    "pma128h4": lambda dev: _pair("pma", 128, 4, torch.float32, dev),
    "pma128h1": lambda dev: _pair("pma", 128, 1, torch.float32, dev),
    "pma128h8": lambda dev: _pair("pma", 128, 8, torch.float32, dev),        # more than 4 heads: the projection without auxiliary rows
    "pma256h4bf16": lambda dev: _pair("pma", 256, 4, torch.bfloat16, dev),
    "deepsets128": lambda dev: _pair("deepsets", 128, 1, torch.float32, dev),
    "linear7": lambda dev: _linear(True, dev),
    "linear7nobias": lambda dev: _linear(False, dev),
    "project_no_bv": _project_without_value_bias,
    "hconv_bias": _hconv,
}

# name -> (queued: [(P, M, [(parameter, offset, shape)])] in queue order, reduced at once: [(reducer, P, M)] in call order)
EXPECTED = {
    'mlp64': ([
        (40, 4288, [('lins.2.weight', 0, (64, 64)), ('lins.2.bias', 4096, (64,)), ('normalizations.2.weight', 4160, (64,)), ('normalizations.2.bias', 4224, (64,))]),
        (40, 4288, [('lins.1.weight', 0, (64, 64)), ('lins.1.bias', 4096, (64,)), ('normalizations.1.weight', 4160, (64,)), ('normalizations.1.bias', 4224, (64,))]),
        (40, 4288, [('lins.0.weight', 0, (64, 64)), ('lins.0.bias', 4096, (64,)), ('normalizations.0.weight', 4160, (64,)), ('normalizations.0.bias', 4224, (64,))]),
    ], []),
    'mlp128': ([
        (19, 16768, [('lins.2.weight', 0, (128, 128)), ('lins.2.bias', 16384, (128,)), ('normalizations.2.weight', 16512, (128,)), ('normalizations.2.bias', 16640, (128,))]),
        (19, 16768, [('lins.1.weight', 0, (128, 128)), ('lins.1.bias', 16384, (128,)), ('normalizations.1.weight', 16512, (128,)), ('normalizations.1.bias', 16640, (128,))]),
        (19, 16768, [('lins.0.weight', 0, (128, 128)), ('lins.0.bias', 16384, (128,)), ('normalizations.0.weight', 16512, (128,)), ('normalizations.0.bias', 16640, (128,))]),
    ], []),
    'mlp256': ([
        (3, 65792, [('lins.2.weight', 0, (256, 256)), ('lins.2.bias', 65536, (256,))]),
        (5, 512, [('normalizations.2.weight', 0, (256,)), ('normalizations.2.bias', 256, (256,))]),
        (3, 65792, [('lins.1.weight', 0, (256, 256)), ('lins.1.bias', 65536, (256,))]),
        (5, 512, [('normalizations.1.weight', 0, (256,)), ('normalizations.1.bias', 256, (256,))]),
        (3, 65792, [('lins.0.weight', 0, (256, 256)), ('lins.0.bias', 65536, (256,))]),
        (5, 512, [('normalizations.0.weight', 0, (256,)), ('normalizations.0.bias', 256, (256,))]),
    ], []),
    'pma128h4': ([
        (19, 16768, [('b.prop.rFF.lins.1.weight', 0, (128, 128)), ('b.prop.rFF.lins.1.bias', 16384, (128,)), ('b.prop.ln1.weight', 16512, (128,)), ('b.prop.ln1.bias', 16640, (128,))]),
        (19, 16896, [('b.prop.rFF.lins.0.weight', 0, (128, 128)), ('b.prop.rFF.lins.0.bias', 16384, (128,)), ('b.prop.ln0.weight', 16512, (128,)), ('b.prop.ln0.bias', 16640, (128,)), ('b.prop.att_r', 16768, (1, 4, 32))]),
        (19, 16512, [('b.prop.lin_V.weight', 0, (128, 128)), ('b.prop.lin_V.bias', 16384, (128,))]),
        (19, 16768, [('a.prop.rFF.lins.1.weight', 0, (128, 128)), ('a.prop.rFF.lins.1.bias', 16384, (128,)), ('a.prop.ln1.weight', 16512, (128,)), ('a.prop.ln1.bias', 16640, (128,))]),
        (19, 16896, [('a.prop.rFF.lins.0.weight', 0, (128, 128)), ('a.prop.rFF.lins.0.bias', 16384, (128,)), ('a.prop.ln0.weight', 16512, (128,)), ('a.prop.ln0.bias', 16640, (128,)), ('a.prop.att_r', 16768, (1, 4, 32))]),
        (19, 16512, [('a.prop.lin_V.weight', 0, (128, 128)), ('a.prop.lin_V.bias', 16384, (128,))]),
    ], [('reduce_partials_slice', 19, 516), ('reduce_partials_to', 19, 516), ('reduce_partials_slice', 19, 516), ('reduce_partials_to', 19, 516)]),
    'pma128h1': ([
        (19, 16768, [('b.prop.rFF.lins.1.weight', 0, (128, 128)), ('b.prop.rFF.lins.1.bias', 16384, (128,)), ('b.prop.ln1.weight', 16512, (128,)), ('b.prop.ln1.bias', 16640, (128,))]),
        (19, 16896, [('b.prop.rFF.lins.0.weight', 0, (128, 128)), ('b.prop.rFF.lins.0.bias', 16384, (128,)), ('b.prop.ln0.weight', 16512, (128,)), ('b.prop.ln0.bias', 16640, (128,)), ('b.prop.att_r', 16768, (1, 1, 128))]),
        (19, 16512, [('b.prop.lin_V.weight', 0, (128, 128)), ('b.prop.lin_V.bias', 16384, (128,))]),
        (19, 16768, [('a.prop.rFF.lins.1.weight', 0, (128, 128)), ('a.prop.rFF.lins.1.bias', 16384, (128,)), ('a.prop.ln1.weight', 16512, (128,)), ('a.prop.ln1.bias', 16640, (128,))]),
        (19, 16896, [('a.prop.rFF.lins.0.weight', 0, (128, 128)), ('a.prop.rFF.lins.0.bias', 16384, (128,)), ('a.prop.ln0.weight', 16512, (128,)), ('a.prop.ln0.bias', 16640, (128,)), ('a.prop.att_r', 16768, (1, 1, 128))]),
        (19, 16512, [('a.prop.lin_V.weight', 0, (128, 128)), ('a.prop.lin_V.bias', 16384, (128,))]),
    ], [('reduce_partials_slice', 19, 516), ('reduce_partials_to', 19, 516), ('reduce_partials_slice', 19, 516), ('reduce_partials_to', 19, 516)]),
    'pma128h8': ([
        (19, 16768, [('b.prop.rFF.lins.1.weight', 0, (128, 128)), ('b.prop.rFF.lins.1.bias', 16384, (128,)), ('b.prop.ln1.weight', 16512, (128,)), ('b.prop.ln1.bias', 16640, (128,))]),
        (19, 16896, [('b.prop.rFF.lins.0.weight', 0, (128, 128)), ('b.prop.rFF.lins.0.bias', 16384, (128,)), ('b.prop.ln0.weight', 16512, (128,)), ('b.prop.ln0.bias', 16640, (128,)), ('b.prop.att_r', 16768, (1, 8, 16))]),
        (19, 16768, [('a.prop.rFF.lins.1.weight', 0, (128, 128)), ('a.prop.rFF.lins.1.bias', 16384, (128,)), ('a.prop.ln1.weight', 16512, (128,)), ('a.prop.ln1.bias', 16640, (128,))]),
        (19, 16896, [('a.prop.rFF.lins.0.weight', 0, (128, 128)), ('a.prop.rFF.lins.0.bias', 16384, (128,)), ('a.prop.ln0.weight', 16512, (128,)), ('a.prop.ln0.bias', 16640, (128,)), ('a.prop.att_r', 16768, (1, 8, 16))]),
    ], [('reduce_partials', 5, 16512), ('reduce_partials', 5, 1032), ('reduce_partials', 5, 16512), ('reduce_partials', 5, 1032)]),
    'pma256h4bf16': ([
        (3, 65792, [('b.prop.rFF.lins.1.weight', 0, (256, 256)), ('b.prop.rFF.lins.1.bias', 65536, (256,))]),
        (3, 65792, [('b.prop.rFF.lins.0.weight', 0, (256, 256)), ('b.prop.rFF.lins.0.bias', 65536, (256,))]),
        (3, 65792, [('b.prop.lin_V.weight', 0, (256, 256)), ('b.prop.lin_V.bias', 65536, (256,))]),
        (3, 65792, [('a.prop.rFF.lins.1.weight', 0, (256, 256)), ('a.prop.rFF.lins.1.bias', 65536, (256,))]),
        (3, 65792, [('a.prop.rFF.lins.0.weight', 0, (256, 256)), ('a.prop.rFF.lins.0.bias', 65536, (256,))]),
        (3, 65792, [('a.prop.lin_V.weight', 0, (256, 256)), ('a.prop.lin_V.bias', 65536, (256,))]),
    ], [('reduce_partials_to', 75, 768), ('reduce_partials_to', 75, 768), ('reduce_partials_slice', 3, 1028), ('reduce_partials_to', 3, 1028), ('reduce_partials_to', 75, 768), ('reduce_partials_to', 75, 768), ('reduce_partials_slice', 3, 1028), ('reduce_partials_to', 3, 1028)]),
    'deepsets128': ([
        (19, 16768, [('b.f_dec.lins.1.weight', 0, (128, 128)), ('b.f_dec.lins.1.bias', 16384, (128,)), ('b.f_dec.normalizations.1.weight', 16512, (128,)), ('b.f_dec.normalizations.1.bias', 16640, (128,))]),
        (19, 16768, [('b.f_dec.lins.0.weight', 0, (128, 128)), ('b.f_dec.lins.0.bias', 16384, (128,)), ('b.f_dec.normalizations.0.weight', 16512, (128,)), ('b.f_dec.normalizations.0.bias', 16640, (128,))]),
        (19, 16768, [('b.f_enc.lins.1.weight', 0, (128, 128)), ('b.f_enc.lins.1.bias', 16384, (128,)), ('b.f_enc.normalizations.1.weight', 16512, (128,)), ('b.f_enc.normalizations.1.bias', 16640, (128,))]),
        (19, 16768, [('b.f_enc.lins.0.weight', 0, (128, 128)), ('b.f_enc.lins.0.bias', 16384, (128,)), ('b.f_enc.normalizations.0.weight', 16512, (128,)), ('b.f_enc.normalizations.0.bias', 16640, (128,))]),
        (19, 16768, [('a.f_dec.lins.1.weight', 0, (128, 128)), ('a.f_dec.lins.1.bias', 16384, (128,)), ('a.f_dec.normalizations.1.weight', 16512, (128,)), ('a.f_dec.normalizations.1.bias', 16640, (128,))]),
        (19, 16768, [('a.f_dec.lins.0.weight', 0, (128, 128)), ('a.f_dec.lins.0.bias', 16384, (128,)), ('a.f_dec.normalizations.0.weight', 16512, (128,)), ('a.f_dec.normalizations.0.bias', 16640, (128,))]),
        (19, 16768, [('a.f_enc.lins.1.weight', 0, (128, 128)), ('a.f_enc.lins.1.bias', 16384, (128,)), ('a.f_enc.normalizations.1.weight', 16512, (128,)), ('a.f_enc.normalizations.1.bias', 16640, (128,))]),
        (19, 16768, [('a.f_enc.lins.0.weight', 0, (128, 128)), ('a.f_enc.lins.0.bias', 16384, (128,)), ('a.f_enc.normalizations.0.weight', 16512, (128,)), ('a.f_enc.normalizations.0.bias', 16640, (128,))]),
    ], []),
    'linear7': ([
        (19, 904, [('weight', 0, (7, 128)), ('bias', 896, (7,))]),
    ], []),
    'linear7nobias': ([
        (19, 904, [('weight', 0, (7, 128))]),
    ], []),
    'project_no_bv': ([
    ], [('reduce_partials', 19, 17028)]),
    'hconv_bias': ([
        (3, 128, [('bias', 0, (128,))]),
    ], [('reduce_partials', 5, 16384)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_the_same_buffers_are_queued_and_the_same_reducers_finish_the_rest(name, device, monkeypatch):
    from allset_amd import dense
    params, run = CASES[name](device)
    names = {id(p): k for k, p in params.items()}

    torch.manual_seed(77)                                      # (the dropout seeds are draws of torch's CPU generator)
    run()
    eager = _grads(params)
    for p in params.values():
        p.grad = None

    queued, reduced = [], []
    real_flush = dense.flush_param_grads
    real = {k: getattr(dense, k) for k in ("reduce_partials", "reduce_partials_to", "reduce_partials_slice")}

    def flush(*a, **k):
        queued.extend((part.shape[0], M, [(names[id(p)], off, tuple(shape)) for p, off, shape in secs])
                      for part, M, secs in dense._Deferred.pending)
        return real_flush(*a, **k)

    def whole(part):
        reduced.append(("reduce_partials", part.shape[0], part[0].numel()))
        return real["reduce_partials"](part)

    def to(part, M, dtype):
        reduced.append(("reduce_partials_to", part.shape[0], M))
        return real["reduce_partials_to"](part, M, dtype)

    def slice_(part, col0, M, dtype):
        reduced.append(("reduce_partials_slice", part.shape[0], M))
        return real["reduce_partials_slice"](part, col0, M, dtype)

    monkeypatch.setattr(dense, "flush_param_grads", flush)
    monkeypatch.setattr(dense, "reduce_partials", whole)
    monkeypatch.setattr(dense, "reduce_partials_to", to)
    monkeypatch.setattr(dense, "reduce_partials_slice", slice_)
    torch.manual_seed(77)
    with dense.deferred_param_grads():
        run()
    monkeypatch.undo()
    print(f"\nCENSUS {name!r}: ({queued!r},\n    {reduced!r}),")
    assert not dense._Deferred.active and not dense._Deferred.pending
    assert (queued, reduced) == EXPECTED[name]
    assert all(P > 1 for P, _, _ in queued), "a family with one partial row decides nothing: raise n for this case"
    got = _grads(params)
    for k, r in eager.items():
        assert (got[k] is None) == (r is None), k
        if r is not None:
            assert got[k].dtype == params[k].dtype and torch.equal(got[k], r), k
