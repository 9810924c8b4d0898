"""CPU: the structure of the exclude-self aggregation without the expansion (incidence.LeaveOneOutIncidence), pinned to
``preprocessing.expand_edge_index`` (whose ids tests/test_preprocessing*.py pin to the reference), ``preprocessing.exclude_self`` and
the driver's choice between the two paths.  The kernels themselves: tests/test_gpu_exclude_self.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from allset_amd import preprocessing as P
from allset_amd.incidence import LeaveOneOutIncidence


def random_hypergraph(seed, n_x=23, n_e=14, with_empty_interior=True):
    """V->E edge list (hyperedge ids from n_x), sorted by vertex: random hyperedges of sizes 2..9, two singletons, one isolated vertex
    (the LAST vertex id, and one in the middle) and one interior hyperedge id without members."""
    rng = np.random.default_rng(seed)
    isolated = {n_x - 1, n_x // 2}
    pairs = []
    for e in range(n_e):
        if with_empty_interior and e == n_e // 2:
            continue                                            # an interior hyperedge id nobody belongs to
        k = 1 if e in (1, n_e - 1) else int(rng.integers(2, 10))
        members = rng.choice([v for v in range(n_x) if v not in isolated], size=k, replace=False)
        pairs += [(int(v), e + n_x) for v in members]
    ei = torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous()
    return SimpleNamespace(edge_index=ei, n_x=torch.tensor([n_x]), num_hyperedges=torch.tensor([n_e]))


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_positions_are_the_expanded_hyperedge_ids(seed):
    data = random_hypergraph(seed)
    n_x = int(data.n_x[0])
    ei = data.edge_index.clone()
    loo = LeaveOneOutIncidence(ei, n_v=n_x, e_base=n_x)
    exp = P.expand_edge_index(SimpleNamespace(**vars(data)))
    ev, ep = exp.edge_index[0], exp.edge_index[1] - n_x             # (vertex, 0-based expanded hyperedge id)
    nnz = ei.shape[1]
    assert loo.nnz == nnz and int(ep.max()) + 1 == nnz               # one expanded hyperedge per incidence
    # the expansion, rebuilt from the structure: position p of the hyperedge-major CSR stands for "its hyperedge without the member
    # at p", so vertex e_col[q] belongs to it for every other position q of the same hyperedge (a singleton keeps its member)
    rp, col = loo.e_rowptr.tolist(), loo.e_col.tolist()
    mine = set()
    for e in range(loo.n_e):
        seg = range(rp[e], rp[e + 1])
        for p in seg:
            for q in seg:
                if q != p or len(seg) == 1:
                    mine.add((col[q], p))
    theirs = set(zip(ev.tolist(), ep.tolist()))
    assert len(theirs) == ev.numel() and mine == theirs
    # members in edge-list order inside a hyperedge, and pos = the position of each incidence of the caller's list
    e0 = ei[1] - n_x
    for j in range(nnz):
        p = int(loo.pos[j])
        assert col[p] == int(ei[0, j]) and rp[int(e0[j])] <= p < rp[int(e0[j]) + 1]
    for e in range(loo.n_e):
        assert loo.pos[(e0 == e)].tolist() == list(range(rp[e], rp[e + 1]))
    # vertex-major CSR: row v lists the positions of v's incidences
    vrp, vcol = loo.v_rowptr.tolist(), loo.v_col.tolist()
    assert len(vrp) == n_x + 1 and vrp[-1] == nnz
    for v in range(n_x):
        assert sorted(vcol[vrp[v]:vrp[v + 1]]) == sorted(loo.pos[ei[0] == v].tolist())
    # sizes and degrees of the expanded graph
    assert torch.equal(loo.row_size[(loo.e_rowptr[1:] - loo.e_rowptr[:-1]).long() > 0].repeat_interleave(
        loo.sizes[loo.sizes > 0]).long(), torch.bincount(ep, minlength=nnz))
    assert torch.equal(loo.vdeg.long(), torch.bincount(ev, minlength=n_x))
    # the reference's sizing rule: the E->V output stops at the largest vertex id with an incidence
    assert loo.n_v == n_x and loo.n_dst == int(ei[0].max()) + 1 < n_x


@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_deg_half_sym_factorises(aggr):
    """norm_contruction('deg_half_sym') on the EXPANDED list is a per-vertex times a per-hyperedge factor; with the mean's 1 / size
    and 1 / degree they are the vectors the structure hands to the kernels."""
    data = random_hypergraph(5)
    n_x = int(data.n_x[0])
    loo = LeaveOneOutIncidence(data.edge_index.clone(), n_v=n_x, e_base=n_x)
    exp = P.norm_contruction(P.expand_edge_index(SimpleNamespace(**vars(data))), option="deg_half_sym")
    ev, ep, norm = exp.edge_index[0], exp.edge_index[1] - n_x, exp.norm.double()
    f = loo.factors(aggr, "deg_half_sym")
    seg_of_pos = torch.repeat_interleave(torch.arange(loo.n_e), loo.sizes)
    size = torch.bincount(ep).double()
    deg = torch.bincount(ev, minlength=n_x).double()
    v2e = f.v2e_src.double()[ev] * f.v2e_seg.double()[seg_of_pos[ep]]
    e2v = f.e2v_row.double()[ev] * f.e2v_seg.double()[seg_of_pos[ep]]
    want_v2e = norm / size[ep] if aggr == "mean" else norm
    want_e2v = norm / deg[ev] if aggr == "mean" else norm
    torch.testing.assert_close(v2e, want_v2e, rtol=4 * 2.0 ** -23, atol=0)
    torch.testing.assert_close(e2v, want_e2v, rtol=4 * 2.0 ** -23, atol=0)
    vpos_vertex = torch.repeat_interleave(torch.arange(n_x), (loo.v_rowptr[1:] - loo.v_rowptr[:-1]).long())
    assert torch.equal(f.e2v_row_inc, f.e2v_row[vpos_vertex]) and torch.equal(f.v2e_src_inc, f.v2e_src[vpos_vertex])
    plain = loo.factors(aggr, "all_one")
    if aggr == "add":
        assert all(t is None for t in plain)
    else:
        assert plain.v2e_src is None and plain.e2v_seg is None
        torch.testing.assert_close(plain.v2e_seg.double()[seg_of_pos[ep]], 1.0 / size[ep], rtol=2.0 ** -23, atol=0)
        torch.testing.assert_close(plain.e2v_row.double()[ev], 1.0 / deg[ev], rtol=2.0 ** -23, atol=0)


def test_duplicates_and_bad_requests_raise():
    ei = torch.tensor([[0, 1, 1, 2], [3, 3, 3, 4]], dtype=torch.int64)
    with pytest.raises(ValueError, match="duplicate"):
        LeaveOneOutIncidence(ei, n_v=3, e_base=3)
    data = SimpleNamespace(edge_index=ei, n_x=[3], num_hyperedges=[2])
    with pytest.raises(ValueError, match="duplicate"):
        P.exclude_self(data)
    ok = torch.tensor([[0, 1, 2], [3, 3, 4]], dtype=torch.int64)
    loo = LeaveOneOutIncidence(ok, n_v=3, e_base=3)
    with pytest.raises(NotImplementedError, match="expand"):
        loo.factors("max", "all_one")
    with pytest.raises(NotImplementedError):
        loo.factors("add", "something_else")
    with pytest.raises(ValueError):
        LeaveOneOutIncidence(ok, n_v=2, e_base=3)                   # vertex id 2 with two vertices
    with pytest.raises(ValueError, match="normtype"):
        P.exclude_self(SimpleNamespace(edge_index=ok, n_x=[3], num_hyperedges=[2]), normtype="nope")
    with pytest.raises(ValueError, match="outside"):
        P.exclude_self(SimpleNamespace(edge_index=ok, n_x=[3], num_hyperedges=[1]))


def test_exclude_self_leaves_the_edge_list_alone():
    data = random_hypergraph(7)
    before = data.edge_index.clone()
    out = P.exclude_self(data, normtype="deg_half_sym")
    assert out is data and torch.equal(data.edge_index, before)
    assert data.exclude_self is True and data.exclude_self_normtype == "deg_half_sym"
    assert data.norm.dtype == torch.int64 and data.norm.shape == (before.shape[1],) and bool((data.norm == 1).all())
    # expand_edge_index is what it was: k (k - 1) incidences per hyperedge of size k > 1, one per singleton
    sizes = torch.bincount(before[1] - int(data.n_x[0]))
    exp = P.expand_edge_index(SimpleNamespace(**vars(random_hypergraph(7))))
    assert exp.edge_index.shape[1] == int((sizes * (sizes - 1)).sum() + (sizes == 1).sum())


def _parse(*argv):
    from allset_amd import train
    args = train.build_parser().parse_args(list(argv))
    args.num_features = 16
    return train, args


def test_driver_picks_the_path():
    train, args = _parse("--exclude_self", "--method", "AllDeepSets")
    assert train.exclude_self_path(args) == "loo"
    train, args = _parse("--exclude_self", "--method", "AllDeepSets", "--normtype", "deg_half_sym", "--MLP_hidden", "512")
    assert train.exclude_self_path(args) == "loo"
    for argv in (["--exclude_self"],                                                        # AllSetTransformer, the default method
                 ["--exclude_self", "--method", "AllSetTransformer"],
                 ["--exclude_self", "--method", "AllDeepSets", "--exclude_self_expand"],
                 ["--exclude_self", "--method", "AllDeepSets", "--normtype", "other"],
                 ["--exclude_self", "--method", "AllDeepSets", "--MLP_hidden", "1024"],     # allset_loo_supported says no
                 ["--exclude_self", "--method", "AllDeepSets", "--MLP_hidden", "66"]):
        train, args = _parse(*argv)
        assert train.exclude_self_path(args) == "expand", argv
    train, args = _parse("--exclude_self", "--method", "AllDeepSets")
    args.LearnMask = True              # (the reference's --LearnMask is store_false over a False default: only code can set it)
    assert train.exclude_self_path(args) == "expand"
    assert not _parse("--method", "AllDeepSets")[1].exclude_self_expand


@pytest.mark.parametrize("expand", [False, True])
def test_driver_preprocess(expand):
    from allset_amd.train import synthetic_dataset
    train, args = _parse("--exclude_self", "--method", "AllDeepSets", *(["--exclude_self_expand"] if expand else []))
    data = train.preprocess(args, synthetic_dataset(feature_noise=1.0, seed=0))
    plain = train.preprocess(_parse("--method", "AllDeepSets")[1], synthetic_dataset(feature_noise=1.0, seed=0))
    if expand:
        assert not getattr(data, "exclude_self", False) and data.edge_index.shape[1] > plain.edge_index.shape[1]
    else:
        assert data.exclude_self and torch.equal(data.edge_index, plain.edge_index) and data.norm.shape == plain.norm.shape
