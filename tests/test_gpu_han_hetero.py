"""GPU: the heterogeneous HAN -- the boolean sparse product of csrc/metapath.hip against scipy with EXACT equality of ``rowptr`` and
``col`` (every bin boundary from both sides, hub rows, an ``n_c`` beyond one LDS bitmap window, chains of one to four relations), its
cross-check against ``han.metapath_edges`` on the synthetic hypergraph, its memory condition and run-to-run bit-identity; the attention
hop of csrc/han.hip on graphs with targets that have no incoming edge (forward and all four gradients against the float64 restatement,
with the product's own attention-dropout factors), and bit-identity with ``han.MetapathGraph`` where no row is empty; the model on the
fixture cases in eval and in training mode (product masks); a 30-epoch run through ``python -m allset_amd.han --hetero``'s ``main``.

Tolerances are tests/test_gpu_han.py's (rtol = atol = 1e-4 against the same kind of float64 restatement), and so is the leaky-relu kink
guard: every comparison asserts, from the restatement alone, that no pre-activation is within 1e-5 of 0; the seeds were fixed on the CPU."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_hetero_cases as hc  # noqa: E402
import han_hetero_oracle as horc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
DEV = torch.device("cuda:0")
BINS = (32, 512, 262144, 256)        # include/allset_hip_ext.h; test_spgemm_cases_cover_the_kernel_paths checks them against the library


def _close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach()
    print(f"{what}: max |diff| {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got, want, msg=lambda m: f"{what}: {m}", **TOL)


def _capture_seeds(monkeypatch):
    from allset_amd import dense
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    return seeds


# ---- the boolean product ---------------------------------------------------------------------------------------------------------
def csr_of(rows, cols, n_rows):
    """(rowptr, col) int64 numpy, duplicates kept, the given order kept within a row."""
    rows, cols = np.asarray(rows, dtype=np.int64), np.asarray(cols, dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64), cols[order]


def _rows_from_lists(lists):
    return [i for i, l in enumerate(lists) for _ in l], [c for l in lists for c in l]


def case_tiny():
    # empty rows of A (1), empty rows of B (2), duplicate entries (A row 0, B row 0), an all-zero result row from a non-empty A row (2)
    a = [[0, 1, 1], [], [2], [3, 0], [1]]
    b = [[0, 4, 4], [2], [], [1, 0]]
    return csr_of(*_rows_from_lists(a), 5), csr_of(*_rows_from_lists(b), 4), 4, 5


def case_random(n_a, n_b, n_c, nnz_a, nnz_b, seed):
    rng = np.random.default_rng(seed)
    return (csr_of(rng.integers(0, n_a, nnz_a), rng.integers(0, n_b, nnz_a), n_a),
            csr_of(rng.integers(0, n_b, nnz_b), rng.integers(0, n_c, nnz_b), n_b), n_b, n_c)


def case_bins():
    """Rows whose candidate count is exactly on and just past each hash-bin boundary, through one entry and through two."""
    rng = np.random.default_rng(5)
    n_c = 1000
    degs = [1, 31, 32, 33, 511, 512, 513, 100, 2]
    b = [list(rng.choice(n_c, size=d, replace=False)) for d in degs]
    a = [[k] for k in range(len(degs))] + [[0, 1], [0, 2], [0, 4], [0, 5], [8, 1], [1, 1], [7, 7, 7, 7, 7, 7], [3, 2, 1, 0]]
    return csr_of(*_rows_from_lists(a), len(a)), csr_of(*_rows_from_lists(b), len(degs)), len(degs), n_c


def case_hub():
    """One middle node with 3000 neighbours on both sides: every row has 3000 candidates and a nearly full result row."""
    n = 3000
    a_rows, a_cols = list(range(n)) + [5, 7], [0] * n + [1, 2]
    b_rows, b_cols = [0] * n + [1, 2, 2], list(range(n)) + [n, n, 3]
    return csr_of(a_rows, a_cols, n + 1), csr_of(b_rows, b_cols, 3), 3, n + 1


def case_wide_rows():
    """Rows of A with 255, 256 and 300 entries over short B rows (the one-entry-per-thread walk and the row just below it)."""
    rng = np.random.default_rng(9)
    n_b, n_c = 400, 700
    b = [list(rng.integers(0, n_c, size=3)) for _ in range(n_b)]
    a = [list(rng.choice(n_b, size=k, replace=False)) for k in (255, 256, 300, 180)]
    return csr_of(*_rows_from_lists(a), len(a)), csr_of(*_rows_from_lists(b), n_b), n_b, n_c


def case_wide_nc():
    """n_c beyond one bitmap window (three windows): bitmap rows through both walks, and hash rows with large column ids."""
    rng = np.random.default_rng(11)
    n_c = 600000
    b = [list(rng.integers(0, n_c, size=700)), list(rng.integers(0, n_c, size=600)), list(rng.integers(200000, 300000, size=20)),
         [n_c - 1, 0, 262143, 262144, 524287, 524288]] + [list(rng.integers(0, n_c, size=2)) for _ in range(300)]
    a = [[0], [1, 0], [2], [3], [2, 3], list(range(4, 304)) + [0], [3] * 100 + [1]]
    return csr_of(*_rows_from_lists(a), len(a)), csr_of(*_rows_from_lists(b), len(b)), len(b), n_c


SPGEMM_CASES = {
    "tiny": case_tiny,
    "rect": lambda: case_random(300, 200, 450, 1500, 1200, 1),
    "square_asymmetric": lambda: case_random(257, 129, 257, 900, 700, 2),
    "dense_rows": lambda: case_random(65, 40, 2000, 600, 8000, 3),
    "bins": case_bins,
    "hub": case_hub,
    "wide_rows": case_wide_rows,
    "wide_nc": case_wide_nc,
}


def _candidates(A, B):
    (rpa, ca), (rpb, _) = A, B
    deg_b = np.diff(rpb)
    return np.array([deg_b[ca[rpa[i]:rpa[i + 1]]].sum() for i in range(rpa.size - 1)]), np.diff(rpa)


def _device_product(A, B, n_c, workspace=None):
    from allset_amd import ops
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(DEV)
    return ops.spgemm_bool(i32(A[0]), i32(A[1]), i32(B[0]), i32(B[1]), n_c, workspace)


@pytest.mark.parametrize("name", sorted(SPGEMM_CASES))
def test_spgemm_equals_scipy_exactly(name):
    A, B, n_b, n_c = SPGEMM_CASES[name]()
    rowptr, col = _device_product(A, B, n_c)
    want_rp, want_col = horc.csr_product(A[0], A[1], B[0], B[1], n_b, n_c)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32
    assert torch.equal(rowptr.cpu().long(), torch.from_numpy(want_rp)), name
    assert torch.equal(col.cpu().long(), torch.from_numpy(want_col)), name
    cand, _ = _candidates(A, B)
    print(f"{name}: {rowptr.numel() - 1} rows, {int(cand.sum())} candidates, {col.numel()} result entries")
    if name == "tiny":
        assert want_rp.tolist() == [0, 3, 3, 3, 6, 7] and want_col.tolist() == [0, 2, 4, 0, 1, 4, 2]
    if name == "square_asymmetric":                          # the direction of the edges is pinned: the transpose is another matrix
        import scipy.sparse as sp
        m = sp.csr_matrix((np.ones(want_col.size), want_col, want_rp), shape=(257, 257))
        assert (m != m.T).nnz > 0
    if name == "hub":
        assert int(np.diff(want_rp)[:3000].min()) == 3000 and want_col.size >= 3000 * 3000


def test_spgemm_cases_cover_the_kernel_paths():
    """Every instantiation is reached, and every bin boundary from both sides: the 16-lane and 64-lane hash tables, the bitmap with one
    window and with several, its two walks (the whole workgroup on a B row / one A entry per thread)."""
    from allset_amd import ops
    assert ops.spgemm_bool_bins() == BINS
    c16, c64, window, wide = BINS
    seen, lens_big, multi = set(), set(), set()
    for name, make in SPGEMM_CASES.items():
        A, B, _, n_c = make()
        cand, len_a = _candidates(A, B)
        seen |= set(int(c) for c in cand)
        for c, l in zip(cand, len_a):
            if c > c64:
                lens_big.add(int(l))
                multi.add((n_c > window, l >= wide))
    assert {0, 1, c16, c16 + 1, c64, c64 + 1} <= seen
    assert wide - 1 in lens_big and wide in lens_big and 1 in lens_big
    assert multi == {(False, False), (False, True), (True, False), (True, True)}
    assert any(make()[3] > window and (_candidates(*make()[:2])[0] <= c16).any() for make in (case_wide_nc,))


def _typed_graph(c):
    from allset_amd.han_hetero import HeteroGraph
    x, edges, num_nodes = hc.raw_data(c)
    g = HeteroGraph({k: (torch.from_numpy(s).to(DEV), torch.from_numpy(d).to(DEV)) for k, (s, d) in edges.items()}, num_nodes)
    return g, horc.TypedGraph(edges, num_nodes), x


@pytest.mark.parametrize("metapath", [["pa"], ["pa", "ap"], ["pf", "fp"], ["ap", "pf"], ["pa", "ap", "pf"], ["fp", "pa", "ap"],
                                      ["pa", "ap", "pf", "fp"], ["ap", "pf", "fp", "pa"]], ids=lambda m: "-".join(m))
def test_metapath_chains_equal_scipy(metapath):
    from allset_amd.han_hetero import metapath_reachable_graph
    g, og, _ = _typed_graph(hc.spec("hetero_h1"))
    rg = metapath_reachable_graph(g, metapath)
    src, dst = horc.reachable_edges(og, metapath)
    _, _, s, d = horc.reachable_csr(og, metapath)
    assert (rg.srctype, rg.dsttype, rg.n_src, rg.n_dst) == (s, d, og.num_nodes[s], og.num_nodes[d])
    assert np.array_equal(rg.src.cpu().numpy(), src) and np.array_equal(rg.dst.cpu().numpy(), dst)
    # both CSR orientations describe these edges
    assert np.array_equal(np.diff(rg.rowptr.cpu().numpy()), np.bincount(dst, minlength=rg.n_dst))
    assert np.array_equal(np.diff(rg.rowptrT.cpu().numpy()), np.bincount(src, minlength=rg.n_src))
    assert rg.zero_in_degree == bool((np.bincount(dst, minlength=rg.n_dst) == 0).any())


def test_layer_refuses_a_metapath_that_ends_on_another_type():
    from allset_amd.han_hetero import HANLayer
    g, _, x = _typed_graph(hc.spec("hetero_h1"))
    layer = HANLayer([["pa", "ap", "pf"]], 12, 4, 1, 0.0).to(DEV)
    with pytest.raises(ValueError, match="leads from 'paper' to 'field'"):
        layer(g, torch.from_numpy(x).float().to(DEV))


def test_cross_check_with_the_hypergraph_metapath_edges():
    """pattern(H H^T) and pattern(H^T H) from the kernel = han.metapath_edges' VEV / EVE lists without their appended loops, edge for
    edge in the same row-major order."""
    from allset_amd import han
    from allset_amd.han_hetero import HeteroGraph, metapath_reachable_graph
    from allset_amd.synthetic import random_hypergraph
    n_v, n_e = 3000, 1200
    hg = random_hypergraph(n_v, n_e, degree=6, seed=4, device=DEV, dist="poisson")
    v, e = hg.edge_index[0], hg.edge_index[1]
    (vr, vc), (er_, ec) = han.metapath_edges(hg.edge_index, n_v, n_e)
    n = n_v + n_e
    g = HeteroGraph({("v", "ve", "e"): (v, e), ("e", "ev", "v"): (e, v)}, {"v": n_v, "e": n_e})
    vev, eve = metapath_reachable_graph(g, ["ve", "ev"]), metapath_reachable_graph(g, ["ev", "ve"])
    assert torch.equal(vev.src, vr[:-n]) and torch.equal(vev.dst, vc[:-n])
    assert torch.equal(eve.src + n_v, er_[:-n]) and torch.equal(eve.dst + n_v, ec[:-n])
    assert vev.nnz > 10 * n_v


def test_memory_stays_proportional_to_the_result():
    """100 papers that all share the same 400 authors: 4 * 10^6 candidate pairs, 10^4 result edges.  The extra device memory of the
    product -- the caller's workspace included -- stays under a tenth of 8 bytes x candidates (the torch expansion needs several times
    8 x candidates; a conforming kernel needs kilobytes)."""
    from allset_amd import ops
    n_p, n_a = 100, 400
    pa = csr_of(np.repeat(np.arange(n_p), n_a), np.tile(np.arange(n_a), n_p), n_p)
    ap = csr_of(np.tile(np.arange(n_a), n_p), np.repeat(np.arange(n_p), n_a), n_a)
    cand, _ = _candidates(pa, ap)
    assert int(cand.sum()) == 4_000_000
    i32 = lambda a: torch.from_numpy(a.astype(np.int32)).to(DEV)
    args = (i32(pa[0]), i32(pa[1]), i32(ap[0]), i32(ap[1]))
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ws = torch.empty(16 + 12 * n_p, dtype=torch.uint8, device=DEV)
    rowptr, col = ops.spgemm_bool(*args, n_p, ws)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    print(f"extra device memory {extra} bytes for {int(cand.sum())} candidates, {col.numel()} result entries")
    assert col.numel() == 10_000 and torch.equal(col.view(n_p, n_p).cpu(), torch.arange(n_p, dtype=torch.int32).expand(n_p, n_p))
    assert extra < 8 * 4_000_000 / 10


def test_two_runs_are_bit_identical():
    for name in ("wide_nc", "dense_rows", "bins"):
        A, B, _, n_c = SPGEMM_CASES[name]()
        r1, c1 = _device_product(A, B, n_c)
        r2, c2 = _device_product(A, B, n_c)
        assert torch.equal(r1, r2) and torch.equal(c1, c2)


# ---- the hop with empty rows -------------------------------------------------------------------------------------------------------
N_HOP = 300
# (heads, channels, attention dropout, seed): the seed is the first of 0, 1, 2, ... whose inputs keep every pre-activation 1e-5 away from
# 0 (found with hop_inputs and the restatement alone, on the CPU)
HOP_CASES = [(1, 5, 0.0, 0), (2, 8, 0.0, 0), (2, 8, 0.6, 0), (8, 8, 0.6, 0), (4, 32, 0.6, 0)]


def hop_inputs(H, C, seed, n=N_HOP, empty=True):
    """A random directed multigraph over ``n`` ids: 4 n random edges, 40 listed twice, a self-loop on every node.  With ``empty``: 30
    targets lose every incoming edge (their loop too), and 10 of those every outgoing edge as well."""
    rng = np.random.default_rng(3000 * seed + 17 * H + C)
    src, dst = rng.integers(0, n, size=4 * n), rng.integers(0, n, size=4 * n)
    src, dst = np.concatenate([src, src[:40], np.arange(n)]), np.concatenate([dst, dst[:40], np.arange(n)])
    if empty:
        gone = rng.choice(n, size=30, replace=False)
        keep = ~np.isin(dst, gone) & ~np.isin(src, gone[:10])
        src, dst = src[keep], dst[keep]
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    return torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64)), f(n, H * C), f(n, H), f(n, H), f(H * C), f(n, H * C)


@pytest.mark.parametrize("case", HOP_CASES, ids=lambda c: f"H{c[0]}C{c[1]}-p{c[2]}")
def test_hop_with_empty_rows_vs_float64(monkeypatch, case):
    from allset_amd.functional import han_edge_keep, han_gat_propagate
    from allset_amd.han_hetero import ReachableGraph
    H, C, p, seed = case
    n = N_HOP
    src, dst, x, el, er, b, G = hop_inputs(H, C, seed)
    deg_in, deg_out = torch.bincount(dst, minlength=n), torch.bincount(src, minlength=n)
    assert int((deg_in == 0).sum()) == 30 and int(((deg_in == 0) & (deg_out == 0)).sum()) == 10
    graph = ReachableGraph(src.to(DEV), dst.to(DEV), n, n)
    assert graph.zero_in_degree
    seeds = _capture_seeds(monkeypatch)
    dv = [t.float().to(DEV).requires_grad_(True) for t in (x, el, er, b)]
    y = han_gat_propagate(dv[0], dv[1], dv[2], graph, H, 0.2, dv[3], p)
    (y * G.float().to(DEV)).sum().backward()
    keep = None
    if p > 0:
        assert len(seeds) == 1
        keep = han_edge_keep(graph, H, p, seeds[0]).cpu().double()
    leaves = [t.clone().requires_grad_(True) for t in (x, el, er, b)]
    rep = []
    yo = horc.gat_hop(src, dst, n, leaves[0], leaves[1], leaves[2], leaves[3], keep, rep)
    (yo * G).sum().backward()
    print(f"min |el[s] + er[t]| = {rep[0]:.3e}")
    assert rep[0] > hc.KINK_MARGIN
    _close(y, yo, "y")
    for got, want, what in zip(dv, leaves, ("gx", "gel", "ger", "gbias")):
        assert bool(torch.isfinite(got.grad).all()), what
        _close(got.grad, want.grad, what)
    # the empty-row rule, exactly: elu(bias) forward; nothing flows into er of such a row, nothing out of a node without edges
    empty = (deg_in == 0).to(DEV)
    assert torch.equal(y.detach()[empty], torch.nn.functional.elu(dv[3].detach()).expand(30, -1))
    assert float(dv[2].grad[empty].abs().max()) == 0.0
    lonely = ((deg_in == 0) & (deg_out == 0)).to(DEV)
    assert float(dv[0].grad[lonely].abs().max()) == 0.0 and float(dv[1].grad[lonely].abs().max()) == 0.0


def test_hop_without_empty_rows_is_bit_identical_to_the_metapath_graph():
    from allset_amd import dense
    from allset_amd.functional import han_gat_propagate
    from allset_amd.han import MetapathGraph
    from allset_amd.han_hetero import ReachableGraph
    H, C, n = 8, 8, N_HOP
    src, dst, x, el, er, b, G = hop_inputs(H, C, 0, empty=False)
    outs = []
    for cls in (lambda: MetapathGraph(src.to(DEV), dst.to(DEV), n), lambda: ReachableGraph(src.to(DEV), dst.to(DEV), n, n)):
        graph = cls()
        for p in (0.0, 0.6):
            torch.manual_seed(5)
            dv = [t.float().to(DEV).requires_grad_(True) for t in (x, el, er, b)]
            y = han_gat_propagate(dv[0], dv[1], dv[2], graph, H, 0.2, dv[3], p)
            (y * G.float().to(DEV)).sum().backward()
            outs.append([y.detach()] + [t.grad for t in dv])
    assert not ReachableGraph(src.to(DEV), dst.to(DEV), n, n).zero_in_degree
    for a, bb in zip(outs[:2], outs[2:]):
        for u, w in zip(a, bb):
            assert torch.equal(u, w)


# ---- model level ---------------------------------------------------------------------------------------------------------------
# training mode: ``torch.manual_seed(MASK_SEED)`` before the forward fixes the product's dropout seeds -- tests/test_gpu_han.py's value
# (its feature masks of [58, 12] contain these cases' [40, 12]); the kink margin is asserted from the restatement fed the resulting masks
MASK_SEED = 1


def _run_model(monkeypatch, name, training):
    from allset_amd import dense
    from allset_amd.functional import han_edge_keep
    from allset_amd.han_hetero import HAN
    c = hc.spec(name)
    g, og, x = _typed_graph(c)
    n = c["n_p"]
    torch.manual_seed(c["seed"])
    model = HAN(meta_paths=hc.META_PATHS, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=hc.DROPOUT)
    model.load_state_dict({k: v.float() for k, v in hc.perturb(model.state_dict(), c).items()})
    sd64 = {k: v.detach().double() for k, v in model.state_dict().items()}               # the fp32 values the device model holds
    model.to(DEV).train(training)
    seeds = _capture_seeds(monkeypatch)
    if training:
        torch.manual_seed(MASK_SEED)
    xd = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
    logits = model(g, xd)
    G = torch.from_numpy(hc.cotangent(c, n))
    (logits * G.float().to(DEV)).sum().backward()
    gs = model.layers[0].reachable_graphs(g)
    edges = [tuple(torch.from_numpy(a) for a in horc.reachable_edges(og, mp)) for mp in hc.META_PATHS]
    for rg, (s, d) in zip(gs, edges):
        assert torch.equal(rg.src.cpu(), s) and torch.equal(rg.dst.cpu(), d)
    assert gs[0].zero_in_degree and not gs[1].zero_in_degree
    assert all(layer.reachable_graphs(g)[0] is layer._cached_coalesced_graph[("pa", "ap")] for layer in model.layers)
    masks = None
    if training:
        assert len(seeds) == 4 * len(c["heads"])                        # per conv: the feature mask, then the attention mask
        masks, k = [], 0
        for l, H in enumerate(c["heads"]):
            width = c["F"] if l == 0 else c["hidden"] * c["heads"][l - 1]
            layer = []
            for rg in gs:
                fk = dense.dropout_scale((n, width), hc.DROPOUT, seeds[k], DEV).cpu().double()
                ek = han_edge_keep(rg, H, hc.DROPOUT, seeds[k + 1]).cpu().double()
                layer.append((fk, ek))
                k += 2
            masks.append(layer)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = torch.from_numpy(x).float().double().requires_grad_(True)
    report = []
    lo = horc.han_forward(sd, edges, n, xo, len(c["heads"]), masks, report)
    (lo * G).sum().backward()
    print(f"{name} training={training}: kink margin {min(report):.3e}")
    assert min(report) > hc.KINK_MARGIN
    _close(logits, lo, "logits")
    _close(xd.grad, xo.grad, "grad_x")
    for k, prm in model.named_parameters():
        _close(prm.grad, sd[k].grad, f"grad:{k}")


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_model_eval_vs_oracle(monkeypatch, name):
    _run_model(monkeypatch, name, training=False)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_model_training_vs_oracle_with_product_masks(monkeypatch, name):
    _run_model(monkeypatch, name, training=True)


def test_gatconv_without_the_flag_raises_on_an_empty_row():
    import torch.nn.functional as F
    from allset_amd.han_hetero import GATConv, ReachableGraph
    graph = ReachableGraph(torch.tensor([0, 1], device=DEV), torch.tensor([1, 1], device=DEV), 2, 2)
    conv = GATConv(4, 2, 1, activation=F.elu).to(DEV)
    with pytest.raises(ValueError, match="0-in-degree"):
        conv(graph, torch.zeros(2, 4, device=DEV))
    out = GATConv(4, 2, 1, activation=F.elu, allow_zero_in_degree=True).to(DEV)(graph, torch.ones(2, 4, device=DEV))
    assert float(out[0].abs().max()) == 0.0                                             # elu(0 + bias), bias = 0 at initialisation


def test_driver_lowers_the_training_loss_in_30_epochs(capsys):
    from allset_amd import han
    args = han.setup(han.build_parser().parse_args(["--hetero", "--dataset", "synthetic", "--runs", "1", "--num_epochs", "30"]).__dict__)
    hist = han.main(args)
    losses = hist["train_loss"][0]
    out = capsys.readouterr().out
    print(f"train loss: first {losses[0]:.4f}, last {losses[-1]:.4f}; test acc {hist['acc'][0]:.2f}")
    assert len(losses) == 30 and losses[-1] < losses[0]
    assert ">> Final test acc:" in out and "test marco f1:" in out and ">> Train time per run:" in out
