"""CPU: the surface of the exclude-self AllSetTransformer path without the expansion -- the driver's choice, the
``attention`` keyword from ``preprocessing.exclude_self`` to ``LooDirection``, the exported symbols -- and, in float64 torch, the
identity the E->V direction rests on.  The kernels themselves: tests/test_gpu_exclude_self_pma.py."""
from types import SimpleNamespace

import numpy as np
import torch

from allset_amd import preprocessing as P
from allset_amd.incidence import LeaveOneOutIncidence, LooDirection


def _hypergraph(name):
    """V->E edge list (hyperedge ids from n_v), sorted by vertex.  'small': 50 vertices, 20 hyperedges of sizes 1..9 (two singletons, the
    last vertex isolated); 'long': one hyperedge of 1025 members among 1100 vertices plus 12 small ones."""
    rng = np.random.default_rng(3)
    if name == "small":
        n_v, sizes = 50, [1, 1] + [int(k) for k in rng.integers(2, 10, size=18)]
    else:
        n_v, sizes = 1100, [1025] + [int(k) for k in rng.integers(1, 7, size=12)]
    pairs = []
    for e, k in enumerate(sizes):
        pairs += [(int(v), e + n_v) for v in rng.choice(n_v - 1, size=k, replace=False)]
    return n_v, len(sizes), torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous()


def _parse(*argv):
    from allset_amd import train
    args = train.build_parser().parse_args(list(argv))
    args.num_features = 16
    return train, args


def test_driver_picks_loo_only_with_the_flag():
    base = ["--exclude_self", "--method", "AllSetTransformer"]
    flag = base + ["--exclude_self_loo_attention"]
    for argv in (flag, flag + ["--heads", "4", "--MLP_hidden", "128"], flag + ["--heads", "8", "--MLP_hidden", "512"],
                 flag + ["--normtype", "other"],                                        # PMA ignores norm
                 ["--exclude_self", "--exclude_self_loo_attention"]):                   # AllSetTransformer is the default method
        train, args = _parse(*argv)
        assert train.exclude_self_path(args) == "loo", argv
    for argv in (base, base + ["--heads", "4", "--MLP_hidden", "128"],                  # without the flag nothing changes
                 flag + ["--exclude_self_expand"],
                 flag + ["--heads", "3", "--MLP_hidden", "96"],                         # heads not built
                 flag + ["--heads", "4", "--MLP_hidden", "24"],                         # C = 6
                 flag + ["--MLP_hidden", "1024"],                                       # too wide
                 flag + ["--heads", "16", "--MLP_hidden", "256"]):
        train, args = _parse(*argv)
        assert train.exclude_self_path(args) == "expand", argv
    train, args = _parse(*flag)
    args.LearnMask = True
    assert train.exclude_self_path(args) == "expand"
    train, args = _parse(*flag)
    args.GPR = True
    assert train.exclude_self_path(args) == "expand"
    # the flag leaves the Deep Sets choice alone
    assert train.exclude_self_path(_parse("--exclude_self", "--method", "AllDeepSets", "--exclude_self_loo_attention")[1]) == "loo"
    assert not _parse("--exclude_self")[1].exclude_self_loo_attention


def test_driver_preprocess_keeps_the_edge_list():
    from allset_amd.train import synthetic_dataset
    train, args = _parse("--exclude_self", "--exclude_self_loo_attention", "--heads", "4", "--MLP_hidden", "128")
    data = train.preprocess(args, synthetic_dataset(feature_noise=1.0, seed=0))
    plain = train.preprocess(_parse("--method", "AllSetTransformer")[1], synthetic_dataset(feature_noise=1.0, seed=0))
    assert data.exclude_self and data.exclude_self_attention and torch.equal(data.edge_index, plain.edge_index)
    expanded = train.preprocess(_parse("--exclude_self")[1], synthetic_dataset(feature_noise=1.0, seed=0))
    assert not getattr(expanded, "exclude_self", False) and expanded.edge_index.shape[1] > plain.edge_index.shape[1]


def test_attention_keyword_round_trips():
    n_v, n_e, ei = _hypergraph("small")
    mk = lambda: SimpleNamespace(edge_index=ei.clone(), n_x=[n_v], num_hyperedges=[n_e])
    assert P.exclude_self(mk()).exclude_self_attention is False
    assert P.exclude_self(mk(), "deg_half_sym").exclude_self_attention is False
    data = P.exclude_self(mk(), attention=True)
    assert data.exclude_self is True and data.exclude_self_attention is True and data.exclude_self_normtype == "all_one"
    loo = LeaveOneOutIncidence(ei, n_v=n_v, e_base=n_v)
    assert LooDirection(loo, "v2e").attention is False and LooDirection(loo, "e2v", "all_one").attention is False
    assert LooDirection(loo, "e2v", "all_one", True).attention is True
    # SetGNN carries the keyword onto both directions
    from allset_amd import SetGNN
    import cases
    model = SetGNN(cases.make_args("pma_h1", 24, 64, 5))
    for want in (False, True):
        pair = model._loo_incidences(ei.clone(), n_v, "all_one", want)
        assert [p.attention for p in pair] == [want, want] and [p.direction for p in pair] == ["v2e", "e2v"]


def test_library_exports_the_new_symbols():
    from allset_amd import _lib, ops
    lib = _lib.load()
    for name in ("allset_loo_softmax_supported", "allset_loo_softmax_fwd", "allset_loo_softmax_bwd"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.allset_version() == 15
    assert ops.loo_softmax_supported(128, 4) and ops.loo_softmax_supported(512, 8) and ops.loo_softmax_supported(4, 1)
    for d, h in ((516, 1), (128, 3), (24, 4), (0, 1), (128, 16), (130, 2)):
        assert not ops.loo_softmax_supported(d, h), (d, h)
    import allset_amd
    assert callable(allset_amd.pma_aggregate_exclude_self)


def test_merging_states_equals_the_softmax_over_the_expanded_list():
    """E->V in float64 torch: per position p = (e, i) the normalised state (o_p, L_p) of e's rows other than the i-th; vertex v's result
    over the EXPANDED list -- the softmax over the union, over v's positions p, of those row sets (disjoint) -- equals
    sum_p exp(L_p) o_p / sum_p exp(L_p)."""
    n_v, n_e, ei = _hypergraph("small")
    loo = LeaveOneOutIncidence(ei, n_v=n_v, e_base=n_v)
    nnz, H, C = loo.nnz, 2, 3
    g = torch.Generator().manual_seed(4)
    a = torch.nn.functional.leaky_relu(2.0 * torch.randn(nnz, H, generator=g, dtype=torch.float64), 0.2)
    y = torch.randn(nnz, H, C, generator=g, dtype=torch.float64)
    # the expanded list: vertex ev attends row ep (a position: the expanded hyperedge's id)
    exp = P.expand_edge_index(SimpleNamespace(edge_index=ei.clone(), n_x=[n_v], num_hyperedges=[n_e]))
    ev, ep = exp.edge_index[0], exp.edge_index[1] - n_v
    want = torch.zeros(loo.n_dst, H, C, dtype=torch.float64)
    for v in range(loo.n_dst):
        rows = ep[ev == v]
        if rows.numel():
            w = torch.softmax(a[rows], dim=0)
            want[v] = (w.unsqueeze(2) * y[rows]).sum(0)
    # stage 1: the state of every position; stage 2: the merge over the vertex-major CSR
    rp = loo.e_rowptr.tolist()
    o, L = torch.zeros(nnz, H, C, dtype=torch.float64), torch.zeros(nnz, H, dtype=torch.float64)
    for e in range(loo.n_e):
        seg = list(range(rp[e], rp[e + 1]))
        for p in seg:
            others = [q for q in seg if q != p] or [p]                 # a singleton keeps its row
            Z = torch.exp(a[others]).sum(0)
            o[p] = (torch.exp(a[others]).unsqueeze(2) * y[others]).sum(0) / Z.unsqueeze(1)
            L[p] = torch.log(Z)
    # position p stands for "e without its i-th member": the vertex AT p does not attend e's rows through p but through every OTHER
    # position of e, and what it gathers there, over all of them, is every row of e but ... its own position's expanded hyperedge.  In
    # the expanded list vertex v (at position p of e) attends the rows q != p of e: exactly the set the state of p holds.
    vrp, vcol = loo.v_rowptr.tolist(), loo.v_col.tolist()
    got = torch.zeros_like(want)
    for v in range(loo.n_dst):
        ps = vcol[vrp[v]:vrp[v + 1]]
        if ps:
            w = torch.softmax(L[ps], dim=0)
            got[v] = (w.unsqueeze(2) * o[ps]).sum(0)
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
