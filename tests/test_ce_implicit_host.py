"""CPU: CEGCN's hop without the clique expansion -- the structure ``preprocessing.ConstructV2V_implicit`` /
``clique_implicit_structure`` derive from the V->E list against what the float64 restatement of the expansion (tests/ce_oracle.py:
``clique_expansion`` + ``gcn_norm``) implies, and the prefix-sum closed form against ``ce_oracle.gcn_conv`` in float64, on the cases
of tests/ce_cases.py."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_cases as cc  # noqa: E402
import ce_oracle as orc  # noqa: E402

D64 = torch.float64
NAMES = sorted(cc.CASES)


def _v2e(name):
    """(V->E list as ExtractV2E leaves it, n_v, x float64)."""
    from allset_amd.preprocessing import ExtractV2E
    c = cc.spec(name)
    x, block, n_v, n_e = cc.raw_data(c)
    data = ExtractV2E(SimpleNamespace(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e]))
    return data.edge_index, n_v, torch.from_numpy(x)


@pytest.fixture(scope="module")
def built():
    """Per case, once: the implicit data and structure, and the oracle's expansion."""
    from allset_amd.preprocessing import ConstructV2V_implicit, clique_implicit_structure
    out = {}
    for name in NAMES:
        ei, n_v, x = _v2e(name)
        data = ConstructV2V_implicit(SimpleNamespace(edge_index=ei.clone()))
        st = clique_implicit_structure(data.edge_index, n_v)
        pairs, mult = orc.clique_expansion(ei)
        out[name] = dict(ei=ei, n_v=n_v, x=x, data=data, st=st, pairs=pairs, mult=mult)
    return out


def prefix_form(x, st, dinv, reverse=False):
    """``dinv[j] * (sum over j's positions of the exclusive prefix (suffix) of dinv * x inside the hyperedge + loop[j] * dinv[j] * x[j])``
    with one cumsum per hyperedge."""
    z = dinv.unsqueeze(1) * x
    rows = z[st["member"]]
    t = torch.zeros_like(rows)
    ptr = st["e_rowptr"].tolist()
    for a, b in zip(ptr[:-1], ptr[1:]):
        if b - a >= 2:
            seg = rows[a:b]
            if reverse:
                t[a:b - 1] = torch.flip(torch.cumsum(torch.flip(seg[1:], [0]), 0), [0])
            else:
                t[a + 1:b] = torch.cumsum(seg[:-1], 0)
    vertex_of_slot = torch.repeat_interleave(torch.arange(st["n"]), st["v_rowptr"][1:] - st["v_rowptr"][:-1])
    acc = torch.zeros_like(x).index_add_(0, vertex_of_slot, t[st["v_pos"]])
    return dinv.unsqueeze(1) * (acc + (st["loop"].to(x.dtype) * dinv).unsqueeze(1) * x)


def _dinv(deg, dtype):
    d = deg.to(dtype).pow(-0.5)
    d[torch.isinf(d)] = 0
    return d


@pytest.mark.parametrize("name", NAMES)
def test_structure_equals_the_expansion(built, name):
    b = built[name]
    st, data, pairs, mult, n_v = b["st"], b["data"], b["pairs"], b["mult"], b["n_v"]
    assert data.clique_expansion is True and data.clique_implicit is True and data.norm is None
    # the data keeps the de-duplicated V->E list, sorted by vertex, hyperedge ids as given
    key = lambda ei: torch.unique(ei[0] * (int(ei.max()) + 1) + ei[1])
    assert data.edge_index.dtype == torch.int64 and torch.equal(key(data.edge_index), key(b["ei"]))
    assert bool((data.edge_index[0][1:] >= data.edge_index[0][:-1]).all())
    nnz = data.edge_index.shape[1]
    member, rank, e_rowptr = st["member"], st["rank"], st["e_rowptr"]
    assert member.numel() == rank.numel() == nnz == int(e_rowptr[-1])
    # members ascend strictly inside a hyperedge; rank = number of smaller members = offset inside the segment
    seg = torch.repeat_interleave(torch.arange(st["n_e"]), e_rowptr[1:] - e_rowptr[:-1])
    same = seg[1:] == seg[:-1]
    assert bool((member[1:][same] > member[:-1][same]).all())
    assert torch.equal(rank, torch.arange(nnz) - e_rowptr[seg])
    # the vertex-major CSR lists every position once, under its own vertex
    assert torch.equal(torch.sort(st["v_pos"]).values, torch.arange(nnz))
    vertex_of_slot = torch.repeat_interleave(torch.arange(n_v), st["v_rowptr"][1:] - st["v_rowptr"][:-1])
    assert torch.equal(member[st["v_pos"]], vertex_of_slot)
    # N, loop, and the integer degree: loop + the multiplicities into j
    N = int(pairs.max()) + 1
    assert st["N"] == N and N < n_v
    assert torch.equal(st["loop"], torch.arange(n_v) < N)
    into = torch.zeros(n_v, dtype=D64).index_add_(0, pairs[1], mult)
    assert st["deg"].dtype == torch.int64 and torch.equal(st["deg"].to(D64), into + st["loop"].to(D64))
    # the pairs the positions stand for are the expansion's, with its multiplicities
    got = {}
    ptr = e_rowptr.tolist()
    for a, e in zip(ptr[:-1], ptr[1:]):
        mem = member[a:e].tolist()
        for hi in range(len(mem)):
            assert int(rank[a + hi]) == hi
            for lo in range(hi):
                got[(mem[lo], mem[hi])] = got.get((mem[lo], mem[hi]), 0) + 1
    assert got == {tuple(p): int(m) for p, m in zip(pairs.t().tolist(), mult.tolist())}
    # dinv[i] * m * dinv[j] reproduces the oracle's weights to float32 rounding (pow and two products: 4 roundings)
    oei, ow = orc.gcn_norm(pairs, mult)
    dinv32 = _dinv(st["deg"], torch.float32)
    m = torch.cat([mult, torch.ones(N, dtype=D64)])
    w32 = (dinv32[oei[0]] * m.float() * dinv32[oei[1]]).to(D64)
    torch.testing.assert_close(w32, ow, rtol=4 * 2.0 ** -23, atol=0)


@pytest.mark.parametrize("name", NAMES)
def test_prefix_form_equals_gcn_conv_in_float64(built, name):
    b = built[name]
    st, x = b["st"], b["x"]
    oei, ow = orc.gcn_norm(b["pairs"], b["mult"])
    # (8 columns: the features through a fixed random projection, so that cora's 1433 columns do not cost a minute)
    x = x @ torch.randn(x.shape[1], 8, generator=torch.Generator().manual_seed(1), dtype=D64)
    eye = torch.eye(8, dtype=D64)
    dinv = _dinv(st["deg"], D64)
    xr = x.clone().requires_grad_(True)
    got = prefix_form(xr, st, dinv)
    want = orc.gcn_conv(x, oei, ow, eye, None)
    torch.testing.assert_close(got.detach(), want, rtol=0, atol=1e-12)
    assert bool((got.detach()[st["N"]:] == 0).all())                     # trailing isolated vertices: nothing arrives, no loop
    G = torch.randn(got.shape, generator=torch.Generator().manual_seed(3), dtype=D64)
    (gx,) = torch.autograd.grad(got, xr, G)
    torch.testing.assert_close(gx, prefix_form(G, st, dinv, reverse=True), rtol=0, atol=1e-12)
    xo = x.clone().requires_grad_(True)
    (go,) = torch.autograd.grad(orc.gcn_conv(xo, oei, ow, eye, None), xo, G)
    torch.testing.assert_close(gx, go, rtol=0, atol=1e-12)


def test_duplicates_offsets_and_singletons():
    from allset_amd.preprocessing import ConstructV2V_implicit, clique_implicit_structure
    ei = torch.tensor([[0, 2, 5, 2, 3, 1, 4], [10, 10, 10, 11, 11, 12, 11]])
    base = clique_implicit_structure(ConstructV2V_implicit(SimpleNamespace(edge_index=ei.clone())).edge_index, 8)
    # duplicates count once
    dup = torch.cat([ei, ei[:, [1, 3, 3]]], dim=1)
    d = ConstructV2V_implicit(SimpleNamespace(edge_index=dup))
    assert d.edge_index.shape[1] == ei.shape[1]
    st = clique_implicit_structure(d.edge_index, 8)
    for k in ("e_rowptr", "member", "rank", "v_rowptr", "v_pos", "deg", "loop"):
        assert torch.equal(st[k], base[k]), k
    # hyperedge ids may be offset arbitrarily (and keep their offset in data.edge_index)
    off = torch.stack([ei[0], ei[1] + 12345])
    d = ConstructV2V_implicit(SimpleNamespace(edge_index=off))
    assert int(d.edge_index[1].min()) == 12355
    st = clique_implicit_structure(d.edge_index, 8)
    for k in ("e_rowptr", "member", "rank", "v_rowptr", "v_pos", "deg", "loop"):
        assert torch.equal(st[k], base[k]), k
    # hand-checked: hyperedges {0, 2, 5}, {2, 3, 4}, {1}; N = 6, vertices 6 and 7 trail
    assert base["N"] == 6 and base["member"].tolist() == [0, 2, 5, 2, 3, 4, 1]
    assert base["deg"].tolist() == [1, 1, 2, 2, 3, 3, 0, 0]
    # only size-1 hyperedges: the expansion is empty, which gcn_norm refuses
    with pytest.raises(ValueError, match="gcn_norm"):
        ConstructV2V_implicit(SimpleNamespace(edge_index=torch.tensor([[0, 1, 2], [5, 6, 7]])))
    with pytest.raises(ValueError, match="gcn_norm"):
        clique_implicit_structure(torch.tensor([[0, 1, 2], [5, 6, 7]]), 3)


def test_driver_flag_and_refusals():
    from allset_amd.train import build_model, build_parser, parse_args
    assert build_parser().parse_args(["--method", "CEGCN"]).CE_implicit is False
    assert parse_args(["--method", "CEGCN", "--CE_implicit"]).CE_implicit is True
    with pytest.raises(SystemExit) as exc:
        parse_args(["--method", "CEGAT", "--CE_implicit"])
    assert exc.value.code == 2
    args = build_parser().parse_args(["--method", "CEGAT"])
    args.num_features, args.num_classes = 4, 2
    data = SimpleNamespace(edge_index=torch.tensor([[0, 1], [2, 2]]), clique_expansion=True, clique_implicit=True, norm=None)
    with pytest.raises(ValueError, match="implicit"):
        build_model(args, data)
