"""GPU: the packed-nonzero-row forward gather (csrc/segreduce.hip pack_rows_kernel / segreduce_packed_kernel).
The packed path must be BITWISE the dense one: every comparison here is an equality of bit patterns."""
import numpy as np
import pytest
import torch

import test_packed_rows_format as fmt

pytestmark = pytest.mark.gpu

SUM, MEAN = 0, 1
DEGREES = (0, 1, 2, 3, 17, 64, 65, 130)     # an empty row, one incidence per slot, an odd count, a full batch, rows crossing 1 and 2 batches


def _bits(t):
    return t.contiguous().view(torch.int32)


def _timed(fn):
    """(fn's result, the names the kernel timer saw)."""
    from allset_amd import ops
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_kernel_timer(None)
    return out, set(timer.events)


# ---- ops.pack_rows against the encoder ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 5, 257])
@pytest.mark.parametrize("strided", [False, True])
def test_pack_rows_matches_the_encoder(n, strided, device):
    from allset_amd import ops
    ks = [fmt.KS[i % len(fmt.KS)] for i in range(n)] if n > 1 else [59]
    for k1 in (fmt.KS if n == 1 else (None,)):
        if k1 is not None:
            ks = [k1]
        x = fmt.make_table(ks, seed=n + 10)
        ref = fmt.encode_rows(x)
        if strided:
            buf = torch.full((n, 192), 3.0, device=device)
            buf[:, :128] = x.to(device)
            xd = buf[:, :128]                                        # ldx = 192 > 128
            assert xd.stride(0) == 192
        else:
            xd = x.to(device)
        got = ops.pack_rows(xd, fmt="mask").cpu()
        assert got.shape == (n, fmt.PITCH_DW) and got.dtype == torch.int32
        assert torch.equal(got[:, :4], ref[:, :4])                   # masks, overflow rows included
        k = torch.tensor(ks)
        defined = (torch.arange(fmt.PITCH_DW)[None, :] < (4 + k)[:, None]) & (k <= fmt.CAP)[:, None]
        assert torch.equal(got[defined], ref[defined])               # values as bit patterns, rows that fit
        assert fmt._same_bits(fmt.decode_rows(got, x), x)


# ---- ops.segreduce_packed against ops.segreduce ------------------------------------------------------------------------------
def _csr(n_rows, n_s, seed):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 9, (n_rows,), generator=g)
    deg[:len(DEGREES)] = torch.tensor(DEGREES)
    deg = deg[torch.randperm(n_rows - 1, generator=g).tolist() + [n_rows - 1]]       # special degrees anywhere but the last row
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    col = torch.randint(0, n_s, (int(rowptr[-1]),), generator=g).to(torch.int32)
    return rowptr, col


def _tables(n_s):
    g = torch.Generator().manual_seed(n_s)
    fit = torch.randint(0, fmt.CAP + 1, (n_s,), generator=g).tolist()
    mix = [int(torch.randint(61, 129, (1,), generator=g)) if i % 10 == 0 else fit[i] for i in range(n_s)]
    around = [fmt.KS[i % len(fmt.KS)] for i in range(n_s)]
    neg0 = fmt.make_table([32] * n_s, seed=5, specials=False)
    neg0[:, ::3] = torch.where(neg0[:, ::3] == 0, torch.full_like(neg0[:, ::3], -0.0), neg0[:, ::3])   # -0.0 where zeros were
    return {
        "fits": fmt.make_table(fit, seed=1, specials=False),
        "mix10": fmt.make_table(mix, seed=2, specials=False),
        "dense": fmt.make_table([128] * n_s, seed=3, specials=False),
        "negative": fmt.make_table(fit, seed=4, specials=False, sign=-1.0),
        "negzero": neg0,
        "capacity_edge": fmt.make_table(around, seed=6, specials=False),
    }


@pytest.mark.parametrize("reduce", [SUM, MEAN])
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("n_s", [1, 300])
def test_segreduce_packed_is_bitwise_the_dense_gather(reduce, ordered, n_s, device):
    from allset_amd import ops
    rowptr, col = _csr(300, n_s, seed=7)
    assert set(DEGREES) <= set((rowptr[1:] - rowptr[:-1]).tolist())
    rowptr, col = rowptr.to(device), col.to(device)
    for name, x in _tables(n_s).items():
        xd = x.to(device)
        packed = ops.pack_rows(xd, fmt="mask")
        for n_t in (300, 299):                                       # 299: not a multiple of the 4 rows of a workgroup
            order = torch.randperm(n_t, generator=torch.Generator().manual_seed(n_t)).to(torch.int32).to(device) if ordered else None
            rp = rowptr[:n_t + 1]
            want, _ = ops.segreduce(reduce, rp, col, None, xd, n_t, variant=1, row_order=order)
            got = ops.segreduce_packed(reduce, rp, col, packed, xd, n_t, row_order=order, fmt="mask")
            assert torch.equal(_bits(got), _bits(want)), (name, n_t)
            empty = (rp[1:] - rp[:-1]) == 0
            assert not _bits(got)[empty].any()                       # empty rows write +0
    if n_s == 300 and not ordered and reduce == SUM:                # and the dense kernel is right about a sum (float64 on the host)
        x = _tables(n_s)["mix10"]
        got = ops.segreduce_packed(SUM, rowptr, col, ops.pack_rows(x.to(device), fmt="mask"), x.to(device), 300, fmt="mask").cpu().double()
        ref = torch.zeros(300, 128, dtype=torch.float64)
        ref.index_add_(0, torch.repeat_interleave(torch.arange(300), (rowptr[1:] - rowptr[:-1]).cpu().long()), x.double()[col.cpu().long()])
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)


# ---- layer level ---------------------------------------------------------------------------------------------------------------
def _hypergraph(device, n_v=500, n_e=400, pairs=4000, seed=3):
    rng = np.random.default_rng(seed)
    p = sorted({(int(rng.integers(n_v)), int(rng.integers(n_e))) for _ in range(pairs)} | {(v, v % n_e) for v in range(n_v)})
    return torch.tensor(p, dtype=torch.int64).t().contiguous().to(device), n_v, n_e


def _conv(device, d=128, dropout=0.5, seed=0):
    from allset_amd import HalfNLHconv
    torch.manual_seed(seed)
    return HalfNLHconv(d, d, d, 2, dropout, "ln", True, attention=False).to(device)


def _run(step, params, x, on):
    """One forward + backward of ``step`` with the packed gather on / off and the dropout seed state brought to the same value."""
    from allset_amd import functional as AF
    was = AF.packed_gather()
    AF.set_packed_gather(on)
    try:
        for p in params:
            p.grad = None
        xs = x.clone().requires_grad_(True)
        torch.manual_seed(11)                                        # dropout seeds are draws from torch's CPU generator
        (out, names) = _timed(lambda: step(xs))
        out.backward(torch.ones_like(out) * 0.5 + out.detach() * 0.25)
        return [out.detach(), xs.grad] + [p.grad.clone() for p in params], names
    finally:
        AF.set_packed_gather(was)


def _assert_same(a, b):
    assert len(a) == len(b)
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.equal(_bits(s), _bits(t)), i


def test_halfnlhconv_training_is_bitwise_unchanged(device):
    from allset_amd import Incidence
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    conv = _conv(device).train()
    x = torch.randn(n_v, 128, device=device)
    params = list(conv.parameters())
    on, names_on = _run(lambda t: conv(t, inc, None, "add"), params, x, True)
    off, names_off = _run(lambda t: conv(t, inc, None, "add"), params, x, False)
    assert "pack_rows" in names_on and "pack_rows" not in names_off      # the switch does switch
    _assert_same(on, off)
    zeros = float((conv._mlp_act(conv.f_enc, x, 0.5) == 0).float().mean())
    assert 0.6 < zeros < 0.9                                             # the gathered table is what the hint says it is


def _sharded_step(device):
    from allset_amd import dist as adist
    ei, n_v, n_e = _hypergraph(device)
    hg = adist.ShardedHypergraph(ei, n_v, n_e, 1, 0).build_incidences()
    a, b = _conv(device, seed=1).train(), _conv(device, seed=2).train()
    params = list(a.parameters()) + list(b.parameters())
    return (lambda t: adist.sharded_deepsets_layer(a, b, t, hg, aggr="add", dropout=0.5, training=True)), params, n_v


def test_sharded_layer_world1_is_bitwise_unchanged(device):
    step, params, n_v = _sharded_step(device)
    x = torch.randn(n_v, 128, device=device)
    on, names_on = _run(step, params, x, True)
    off, names_off = _run(step, params, x, False)
    assert "pack_rows" in names_on and "pack_rows" not in names_off
    _assert_same(on, off)


def test_layer_step_replays_from_a_graph(device):
    """The packed path decides from its arguments alone (no data pass, no host sync): the layer step captures into one graph, and the
    replay equals the eager step under the same seed counter."""
    from allset_amd import dense
    from allset_amd import functional as AF
    from allset_amd.graphs import _side_stream_warmup
    assert AF.packed_gather()
    step, params, n_v = _sharded_step(device)
    x = torch.randn(n_v, 128, device=device, requires_grad=True)
    counter = torch.full((1,), 5, dtype=torch.int64, device=device)

    G = torch.ones(n_v, 128, device=device)

    def fwd_bwd():
        for p in params:
            p.grad = None
        x.grad = None
        out = step(x)
        with dense.deferred_param_grads():                           # as the training driver and the benchmark run their step
            out.backward(G)
        return out

    # Capture FIRST, as graphs.GraphedTrainStep does (warm-up on a side stream, capture on that stream).  The eager step comes last: an
    # eager backward on the default stream before the capture would leave the leaves' gradient accumulators bound to the default
    # stream for as long as its output lives, and the captured backward would then reach across to a stream that is not capturing.
    with torch.cuda.device(device):
        with dense.device_seed_counter(counter):                     # the salts restart at every entry: same masks in all three
            st = _side_stream_warmup(fwd_bwd, 2)
        graph = torch.cuda.CUDAGraph()
        with dense.device_seed_counter(counter), torch.cuda.graph(graph, stream=st):
            out = fwd_bwd()
    graph.replay()
    torch.cuda.synchronize()
    replayed = [out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params]
    del out                                                          # (with it goes the captured autograd graph and its accumulators)
    with dense.device_seed_counter(counter):
        out = fwd_bwd()
    _assert_same([out.detach(), x.grad] + [p.grad for p in params], replayed)


# ---- dispatch: everything else keeps today's path --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["weights", "max", "bf16", "d64"])
def test_hint_falls_back_outside_the_built_shape(case, device):
    from allset_amd import Incidence
    from allset_amd import functional as AF
    assert AF.packed_gather()
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    d = 64 if case == "d64" else 128
    x = torch.relu(torch.randn(n_v, d, device=device)) * (torch.rand(n_v, d, device=device) < 0.5)
    if case == "bf16":
        x = x.to(torch.bfloat16)
    norm = (torch.rand(ei.shape[1], device=device) + 0.5) if case == "weights" else None
    aggr = "max" if case == "max" else "add"
    plain = AF.deepsets_aggregate(x, inc, norm, aggr)
    hinted, names = _timed(lambda: AF.deepsets_aggregate(x, inc, norm, aggr, packed_rows=True))
    assert "pack_rows" not in names and "segreduce_fwd" in names
    assert torch.equal(hinted, plain)


def test_hint_takes_the_packed_path_at_the_built_shape(device):
    from allset_amd import Incidence
    from allset_amd import functional as AF
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    x = torch.relu(torch.randn(n_v, 128, device=device)) * (torch.rand(n_v, 128, device=device) < 0.5)
    for aggr in ("add", "mean"):
        plain = AF.deepsets_aggregate(x, inc, None, aggr)
        hinted, names = _timed(lambda: AF.deepsets_aggregate(x, inc, None, aggr, packed_rows=True))
        assert "pack_rows" in names
        assert torch.equal(_bits(hinted), _bits(plain))


def test_eval_mode_keeps_the_dense_gather(device):
    from allset_amd import Incidence
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    conv = _conv(device).eval()
    x = torch.randn(n_v, 128, device=device)
    on, names_on = _run(lambda t: conv(t, inc, None, "add"), list(conv.parameters()), x, True)
    off, _ = _run(lambda t: conv(t, inc, None, "add"), list(conv.parameters()), x, False)
    assert "pack_rows" not in names_on
    _assert_same(on, off)
