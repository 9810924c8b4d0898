"""GPU: the fused Linear forward that writes cell rows from its own epilogue (csrc/fused_fwd2.hip mode 4) against
the pair it replaces -- the dense kernel's output and ``ops.pack_rows(., fmt="cells")`` of it -- and the layers under the three routes of the forward
gather: cell rows, mask rows, dense.  Every comparison is an equality of bit patterns."""
import numpy as np
import pytest
import torch

import test_cell_rows_format as fmt
from test_gpu_cell_gather import _bits, _formats, _hypergraph, _restore, _timed

pytestmark = pytest.mark.gpu

# 1; a partial four-row group; the 32-row stage boundary; several stages; 4099 rows: 129 stages, the last of 3 rows
ROWS = (1, 31, 32, 33, 500, 4099)
TABLES = ("near32", "block", "sparse")
SENTINEL = 0x7FC12345                       # a NaN payload no kernel produces: "this row of the side table was not written"


def _params(table, device):
    """(W, bias, gamma, beta).  With dropout 0.5 in and out:
    near32 -- small random biases: about half the columns survive the relu, k ~ Bin(128, 1/4), rows around 32, a few above 48;
    block  -- +6 on 100 columns, -6 on the rest (against Linear terms of standard deviation < 0.4: no relu flips): k ~ Bin(100, 1/2),
              rows on both sides of 48, about 57 % above it;
    sparse -- +6 on 3 columns, -6 on the rest: k ~ Bin(3, 1/2), one row in eight all zero."""
    g = torch.Generator().manual_seed(17)
    W = torch.randn(128, 128, generator=g) / 128 ** 0.5
    gamma = 1.0 + 0.1 * torch.randn(128, generator=g)
    beta = 0.1 * torch.randn(128, generator=g)
    if table == "near32":
        bias = 0.1 * torch.randn(128, generator=g)
    else:
        W = 0.25 * W
        bias = torch.full((128,), -6.0)
        bias[torch.randperm(128, generator=g)[:100 if table == "block" else 3]] = 6.0
    return [t.to(device) for t in (W, bias, gamma, beta)]


def _cells_linear(x, W, bias, gamma, beta, arith, mask, device):
    """ops.fused_linear_fwd_packed(..., fmt="cells") through the C entry point, with a side table the test filled beforehand."""
    from allset_amd import _lib
    n = x.shape[0]
    cells = torch.empty(n, fmt.PITCH_DW, dtype=torch.int32, device=device)
    side = torch.full((n, 128), SENTINEL, dtype=torch.int32, device=device)
    stats = torch.empty(n, 2, device=device)
    _lib.check(_lib.load().allset_fused_linear_fwd_cells(
        _lib.ptr(x), 128, _lib.ptr(gamma), _lib.ptr(beta), 1e-5, 1, 0.5, 101, _lib.ptr(W), _lib.ptr(bias), 1, 0.5, 202, _lib.ptr(cells),
        _lib.ptr(side), 128, _lib.ptr(stats), n, 128, 128, None, _lib.ptr(mask), int(arith), _lib.stream_of(device)),
        "allset_fused_linear_fwd_cells")
    return cells, side, stats


@pytest.mark.parametrize("table", TABLES)
@pytest.mark.parametrize("arith", ["fp16x3", "bf16x6"])
def test_cell_epilogue_equals_linear_then_pack_cells(arith, table, device):
    from allset_amd import dense, ops
    W, bias, gamma, beta = _params(table, device)
    for n in ROWS:
        x = torch.randn(n, 128, generator=torch.Generator().manual_seed(n)).to(device)
        words = dense.activation_mask_words(n, 128)
        m_ref = torch.zeros(words, dtype=torch.int32, device=device)
        m_new = torch.zeros(words, dtype=torch.int32, device=device)
        with dense.arithmetic(arith):
            y, stats = dense.fused_linear_fwd(x, W, bias, gamma, beta, 1e-5, True, 0.5, 101, True, 0.5, 202, None, m_ref)
            cells, side, stats_new = _cells_linear(x, W, bias, gamma, beta, dense._arith_for(0, 128, 128, True, 0), m_new, device)
        want = ops.pack_rows(y, fmt="cells")
        assert torch.equal(cells, want), (n, "cell rows")
        assert torch.equal(want.cpu(), torch.from_numpy(fmt.encode_cells(y.cpu().numpy()).view(np.int32))), (n, "the reference's own rows")
        k = (_bits(y) != 0).sum(1)
        over = k > fmt.CAP
        assert torch.equal(side[over], _bits(y)[over]), (n, "side table on the overflow rows")
        assert bool((side[~over] == SENTINEL).all()), (n, "no other row of the side table is written")
        assert torch.equal(m_new, m_ref), (n, "1-bit activation mask")
        assert torch.equal(_bits(stats_new), _bits(stats)), (n, "row statistics")
        print(f"{table} {arith} n={n}: k mean {float(k.float().mean()):.1f} min {int(k.min())} max {int(k.max())}, above 48: {int(over.sum())}")
        if n == 4099:                                                    # the table holds what it is meant to hold
            if table == "near32":
                assert 28 <= float(k.float().mean()) <= 36 and int(((k >= 30) & (k <= 34)).sum()) > 500
            if table == "block":
                assert 0.3 <= float(over.float().mean()) <= 0.8 and int((k == 48).sum()) > 0 and int((k == 49).sum()) > 0
            if table == "sparse":
                assert int((k == 0).sum()) > 100 and int(k.max()) == 3


@pytest.mark.parametrize("table", TABLES)
def test_gather_over_the_cell_epilogue_is_the_dense_gather(table, device):
    from allset_amd import dense, ops
    n_s = 4099
    W, bias, gamma, beta = _params(table, device)
    x = torch.randn(n_s, 128, generator=torch.Generator().manual_seed(3)).to(device)
    mask = torch.zeros(dense.activation_mask_words(n_s, 128), dtype=torch.int32, device=device)
    y, _ = dense.fused_linear_fwd(x, W, bias, gamma, beta, 1e-5, True, 0.5, 101, True, 0.5, 202, None, mask)
    cells, side, _ = ops.fused_linear_fwd_packed(x, W, bias, gamma, beta, 1e-5, True, 0.5, 101, True, 0.5, 202, None, mask,
                                                 dense._arith_for(0, 128, 128, True, 0), fmt="cells")
    g = torch.Generator().manual_seed(9)
    deg = torch.randint(0, 40, (301,), generator=g)
    rowptr = torch.zeros(302, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    col = torch.randint(0, n_s, (int(rowptr[-1]),), generator=g).to(torch.int32)
    rowptr, col = rowptr.to(device), col.to(device)
    want, _ = ops.segreduce(0, rowptr, col, None, y, 301, variant=1)
    assert torch.equal(_bits(ops.segreduce_packed(0, rowptr, col, cells, side, 301, fmt="cells")), _bits(want))


# ---- layer level: cell rows, mask rows and the dense gather give the same training step ----------------------------------------
ROUTES = (("cells", True), ("mask", True), ("cells", False))            # (format, packed gather on)


def _conv(device, seed=0):
    from allset_amd import HalfNLHconv
    torch.manual_seed(seed)
    return HalfNLHconv(128, 128, 128, 2, 0.5, "ln", True, attention=False).to(device)


class _route:
    def __init__(self, fmt_name, gather_on, epilogue):
        self.to = (fmt_name, gather_on, epilogue)

    def __enter__(self):
        from allset_amd import functional as AF
        self.was = (_formats(), AF.packed_gather(), AF.packed_epilogue())
        AF.set_packed_format(self.to[0]); AF.set_packed_gather(self.to[1]); AF.set_packed_epilogue(self.to[2])

    def __exit__(self, *exc):
        from allset_amd import functional as AF
        _restore(self.was[0]); AF.set_packed_gather(self.was[1]); AF.set_packed_epilogue(self.was[2])


def _run(step, params, x):
    for p in params:
        p.grad = None
    xs = x.clone().requires_grad_(True)
    torch.manual_seed(11)                                                # dropout seeds are draws from torch's CPU generator
    (out, names) = _timed(lambda: step(xs))
    out.backward(torch.ones_like(out) * 0.5 + out.detach() * 0.25)
    return [out.detach(), xs.grad] + [p.grad.clone() for p in params], names


def _assert_same(a, b):
    assert len(a) == len(b)
    for i, (s, t) in enumerate(zip(a, b)):
        assert torch.equal(s, t), i


def _layer_steps(device):
    from allset_amd import Incidence
    from allset_amd import dist as adist
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    conv = _conv(device).train()
    hg = adist.ShardedHypergraph(ei, n_v, n_e, 1, 0).build_incidences()
    a, b = _conv(device, seed=1).train(), _conv(device, seed=2).train()
    return {"halfnlhconv": ((lambda t: conv(t, inc, None, "add")), list(conv.parameters())),
            "sharded": ((lambda t: adist.sharded_deepsets_layer(a, b, t, hg, aggr="add", dropout=0.5, training=True)),
                        list(a.parameters()) + list(b.parameters()))}, n_v


@pytest.mark.parametrize("layer", ["halfnlhconv", "sharded"])
@pytest.mark.parametrize("epilogue", ["on", "off"])
def test_training_step_is_the_same_under_every_route(layer, epilogue, device):
    steps, n_v = _layer_steps(device)
    step, params = steps[layer]
    x = torch.randn(n_v, 128, device=device)
    res = {}
    for route in ROUTES:
        with _route(*route, epilogue):
            res[route] = _run(step, params, x)
    for route in ROUTES[:2]:
        names = res[route][1]
        assert "segreduce_fwd" in names and "fused_linear_fwd" in names and (("pack_rows" in names) == (epilogue == "off")), route
    assert "pack_rows" not in res[ROUTES[2]][1]
    _assert_same(res[ROUTES[0]][0], res[ROUTES[2]][0])
    _assert_same(res[ROUTES[1]][0], res[ROUTES[2]][0])


def test_default_routes_of_the_sharded_layer(device, monkeypatch):
    """By default the V->E half gathers mask rows and the E->V half cell rows, each written by its own Linear."""
    from allset_amd import functional as AF
    from allset_amd import ops
    steps, n_v = _layer_steps(device)
    step, _ = steps["sharded"]
    calls = []
    for name in ("segreduce_packed", "fused_linear_fwd_packed", "pack_rows"):
        monkeypatch.setattr(ops, name, (lambda fn, name: lambda *a, **k: (calls.append((name, k["fmt"])), fn(*a, **k))[1])(getattr(ops, name), name))
    was = AF.packed_epilogue()
    AF.set_packed_epilogue("on")
    try:
        step(torch.randn(n_v, 128, device=device))
    finally:
        AF.set_packed_epilogue(was)
    assert calls == [("fused_linear_fwd_packed", "mask"), ("segreduce_packed", "mask"), ("fused_linear_fwd_packed", "cells"), ("segreduce_packed", "cells")]


def test_every_route_replays_the_same_from_a_graph(device):
    """Each route captures into one graph; three replays under fresh dropout counters give, route by route, the same step."""
    from allset_amd import dense
    from allset_amd.graphs import _side_stream_warmup
    steps, n_v = _layer_steps(device)
    step, params = steps["sharded"]
    x = torch.randn(n_v, 128, device=device, requires_grad=True)
    counter = torch.full((1,), 5, dtype=torch.int64, device=device)
    G = torch.ones(n_v, 128, device=device)

    def fwd_bwd():
        for p in params:
            p.grad = None
        x.grad = None
        out = step(x)
        with dense.deferred_param_grads():
            out.backward(G)
        return out

    replays = {}
    for route in ROUTES:
        with _route(*route, "on"):
            counter.fill_(5)
            with torch.cuda.device(device):
                with dense.device_seed_counter(counter):
                    st = _side_stream_warmup(fwd_bwd, 2)
                graph = torch.cuda.CUDAGraph()
                with dense.device_seed_counter(counter), torch.cuda.graph(graph, stream=st):
                    out = fwd_bwd()
            got = []
            for i in range(3):
                counter.fill_(40 + i)                                    # a fresh dropout counter per replay
                graph.replay()
                torch.cuda.synchronize()
                got.append([out.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in params])
            replays[route] = got
            del out, graph
    for i in range(3):
        _assert_same(replays[ROUTES[0]][i], replays[ROUTES[2]][i])
        _assert_same(replays[ROUTES[1]][i], replays[ROUTES[2]][i])
    assert not torch.equal(replays[ROUTES[0]][0][0], replays[ROUTES[0]][1][0])      # the counters did change the masks
