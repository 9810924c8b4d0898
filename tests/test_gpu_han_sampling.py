"""GPU: mini-batch HAN -- the metapath random-walk sampler (csrc/han_sample.hip, allset_amd/han_sampling.py): bit-identity for equal
(seed, counter), a node's row independent of its batch, validity of every block against the dense ``H H^T`` / ``H^T H`` restatement,
the endpoint distribution of the raw walks and the collision rate of two walk lanes against the exact values under the binomial
5-sigma bound; the bipartite hop forward and backward against the float64 restatement of tests/han_sampling_oracle.py with the
product's own attention-dropout factors; the whole model on the fixed blocks of tests/han_sampling_cases.py against the restatement
AND the recorded reference at the suite's fp32 parity level, rtol = atol = 1e-4, in eval mode and in training mode (product masks);
a square block against ``han_gat_propagate`` and a stacked buffer over a non-square block against separate calls, bit for bit; error paths (argument checks only); the driver twice, bit for bit, and its
training loss over a short synthetic run.

The leaky-relu kink: as in tests/test_gpu_han.py, every comparison asserts from the float64 restatement alone that the nearest
pre-activation is more than 1e-5 away from 0; the seeds were fixed on the CPU so that it is."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_sampling_cases as sc  # noqa: E402
import han_sampling_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)
DEV = torch.device("cuda:0")


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


# ---- sampler -------------------------------------------------------------------------------------------------------------------
def _walker(name="hs_h2"):
    from allset_amd.han_sampling import MetapathWalker
    c = sc.spec(name)
    _, pairs, n_v, n_e = sc.raw_data(c)
    data = SimpleNamespace(edge_index=torch.from_numpy(pairs).to(DEV), n_x=[n_v], num_hyperedges=[n_e])
    return c, pairs, n_v, n_e, MetapathWalker(data)


def _rows(block):
    """{global target id: [global source ids in slot order]} of a sampled block."""
    rp, col, ids = block.rowptr.cpu().numpy(), block.col.cpu().numpy(), block.src_ids.cpu().numpy()
    return {int(ids[t]): [int(ids[s]) for s in col[rp[t]:rp[t + 1]]] for t in range(block.n_dst)}


def _block_tensors(b):
    return [b.src_ids, b.src, b.dst, b.rowptr, b.col, b.perm, b.rowptrT, b.colT, b.slotT]


def test_equal_seed_and_counter_are_bit_identical_and_counters_differ():
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HANSampler, random_walk_endpoints
    c, pairs, n_v, n_e, w = _walker()
    seeds = list(range(0, 30)) + [n_v - 1, n_v + 2, n_v + 7]
    a = HANSampler(w, DEFAULT_METAPATHS, 8, seed=4).sample_blocks(seeds, counter=9)[1]
    b = HANSampler(w, DEFAULT_METAPATHS, 8, seed=4).sample_blocks(seeds, counter=9)[1]
    d = HANSampler(w, DEFAULT_METAPATHS, 8, seed=4).sample_blocks(seeds, counter=10)[1]
    e = HANSampler(w, DEFAULT_METAPATHS, 8, seed=5).sample_blocks(seeds, counter=9)[1]
    for x, y in zip(a, b):
        assert (x.n_src, x.n_dst, x.nnz) == (y.n_src, y.n_dst, y.nnz)
        assert all(torch.equal(s, t) for s, t in zip(_block_tensors(x), _block_tensors(y)))
    assert _rows(a[0]) != _rows(d[0]) and _rows(a[1]) != _rows(d[1])
    assert _rows(a[0]) != _rows(e[0])
    r1 = random_walk_endpoints(w, 'VEV', seeds, 16, 4, 9)
    assert r1.dtype == torch.int64 and tuple(r1.shape) == (len(seeds), 16)
    assert torch.equal(r1, random_walk_endpoints(w, ['Vs_E', 'E_Vs'], torch.tensor(seeds, device=DEV), 16, 4, 9))
    assert not torch.equal(r1, random_walk_endpoints(w, 'VEV', seeds, 16, 4, 10))
    s = HANSampler(w, DEFAULT_METAPATHS, 8, seed=4)                              # the sampler's own counter advances per call
    first, second = s.sample_blocks(seeds)[1], s.sample_blocks(seeds)[1]
    assert s.counter == 2 and _rows(first[0]) != _rows(second[0])


def test_a_nodes_row_does_not_depend_on_its_batch():
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HANSampler
    c, pairs, n_v, n_e, w = _walker()
    s = HANSampler(w, DEFAULT_METAPATHS, 6, seed=2)
    batch1 = [3, 17, 5, n_v + 4, 20, 1]
    batch2 = [n_v + 4, 30, 5, 9, 3, 11, 12, 13, 14]
    b1, b2 = s.sample_blocks(batch1, counter=3)[1], s.sample_blocks(batch2, counter=3)[1]
    for x, y in zip(b1, b2):
        r1, r2 = _rows(x), _rows(y)
        for node in (3, 5, n_v + 4):
            assert r1[node] == r2[node] and len(r1[node]) >= 1


@pytest.mark.parametrize("name,k,B", [("hs_h2", 5, 20), ("hs_h2", 64, 58), ("cora_hs", 20, 1024)])
def test_blocks_are_valid_against_the_dense_restatement(name, k, B):
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HANSampler, load_subtensors
    c, pairs, n_v, n_e, w = _walker(name)
    Hm = np.zeros((n_v, n_e))
    Hm[pairs[0], pairs[1]] = 1.0
    n = n_v + n_e
    adj = [np.zeros((n, n), dtype=bool), np.zeros((n, n), dtype=bool)]
    adj[0][:n_v, :n_v] = (Hm @ Hm.T) > 0
    adj[1][n_v:, n_v:] = (Hm.T @ Hm) > 0
    seeds = np.random.default_rng(1).choice(n, size=B, replace=False)            # vertices (isolated ones too) and hyperedge nodes
    got_seeds, blocks = HANSampler(w, DEFAULT_METAPATHS, k, seed=1).sample_blocks(seeds.tolist(), counter=0)
    assert list(got_seeds) == seeds.tolist() and len(blocks) == 2
    feats = load_subtensors(blocks, torch.arange(n, device=DEV).float().view(-1, 1))
    some_neighbours = [False, False]
    for mp, b in enumerate(blocks):
        ids = b.src_ids.cpu().numpy()
        assert b.n_dst == B and np.array_equal(ids[:B], seeds) and len(set(ids.tolist())) == b.n_src == ids.size
        assert np.array_equal(ids[B:], np.sort(ids[B:]))                         # the non-seed nodes ascending
        assert np.array_equal(feats[mp].cpu().numpy()[:, 0], ids.astype(np.float32))
        rows = _rows(b)
        used = set()
        for s in seeds.tolist():
            r = rows[s]
            assert r[-1] == s and s not in r[:-1]                                # one self-loop, last
            assert r[:-1] == sorted(set(r[:-1])) and len(r) - 1 <= k             # distinct, ascending, at most k
            assert all(adj[mp][s, u] for u in r[:-1])                            # every neighbour shares a hyperedge / a vertex
            if not adj[mp][s].any():
                assert r == [s]                                                  # no out-edges: the self-loop alone
            some_neighbours[mp] |= len(r) > 1
            used |= set(r)
        assert used == set(ids.tolist())                                         # no source node without an edge
        # the edge list, both CSR orientations and slotT describe the same multiset of edges
        src, dst = b.src.cpu().numpy(), b.dst.cpu().numpy()
        rp, col, perm = b.rowptr.cpu().numpy(), b.col.cpu().numpy(), b.perm.cpu().numpy()
        assert b.nnz == src.size == rp[-1] and rp[0] == 0
        slot_dst = np.repeat(np.arange(B), np.diff(rp))
        assert np.array_equal(src[perm], col) and np.array_equal(dst[perm], slot_dst)
        rpT, colT, slotT = b.rowptrT.cpu().numpy(), b.colT.cpu().numpy(), b.slotT.cpu().numpy()
        assert rpT.size == b.n_src + 1 and rpT[0] == 0 and rpT[-1] == b.nnz
        srcT = np.repeat(np.arange(b.n_src), np.diff(rpT))
        assert sorted(slotT.tolist()) == list(range(b.nnz))
        assert np.array_equal(col[slotT], srcT) and np.array_equal(slot_dst[slotT], colT)
    assert all(some_neighbours)
    vertex_seeds = [s for s in seeds.tolist() if s < n_v]
    assert all(_rows(blocks[1])[s] == [s] for s in vertex_seeds)                 # EVE from a vertex: the self-loop alone (kept)


def test_walk_endpoints_follow_the_exact_distribution_and_lanes_are_independent():
    from allset_amd.han_sampling import random_walk_endpoints
    c, pairs, n_v, n_e, w = _walker()
    v2e, e2v = orc.adjacency(pairs, n_v, n_e)
    k, counters = 64, 256
    N = k * counters
    for mp, seeds in ((0, [0, 1, 2, 7, 19, 33, n_v - 1, n_v + 1]), (1, [n_v, n_v + 1, n_v + 4, n_v + 9, n_v + 17, 3])):
        walks = torch.stack([random_walk_endpoints(w, mp, seeds, k, 12345, ctr) for ctr in range(counters)]).cpu().numpy()
        assert walks.shape == (counters, len(seeds), k)
        for i, s in enumerate(seeds):
            p = orc.endpoint_distribution(v2e, e2v, n_v, mp, s)
            ends = walks[:, i, :]
            if not p:
                assert (ends == -1).all()                                        # no out-edges: every walk terminates
                continue
            assert set(np.unique(ends).tolist()) <= set(p), (mp, s)
            worst = 0.0
            for u, pu in p.items():
                f = float((ends == u).mean())
                bound = 5 * np.sqrt(pu * (1 - pu) / N)
                worst = max(worst, abs(f - pu) / bound)
                assert abs(f - pu) <= bound, (mp, s, u, f, pu, bound)
            # two different walk lanes of one seed collide with probability sum p^2 if they are independent
            q = sum(v * v for v in p.values())
            hits = (ends[:, 0::2] == ends[:, 1::2])
            n_pairs = hits.size
            fq = float(hits.mean())
            qb = 5 * np.sqrt(q * (1 - q) / n_pairs) if q < 1 else 0.0
            print(f"metapath {mp} seed {s}: {len(p)} endpoints, worst |f - p| / bound {worst:.2f}; collisions {fq:.4f} vs {q:.4f} +- {qb:.4f}")
            assert abs(fq - q) <= qb, (mp, s, fq, q, qb)
            # ... and so do the same lane at two consecutive counters
            hits = (ends[0::2, :] == ends[1::2, :])
            assert abs(float(hits.mean()) - q) <= (5 * np.sqrt(q * (1 - q) / hits.size) if q < 1 else 0.0), (mp, s)


# ---- hop -----------------------------------------------------------------------------------------------------------------------
N_DST, N_SRC = 300, 900
# (heads, channels, attention dropout, long rows, seed): the seed is the first of 0, 1, 2, ... whose inputs keep every pre-activation
# 1e-5 away from 0 (found with hop_inputs and the restatement alone, on the CPU).  H * C = 1 and 512 are the two ends of the
# VEC / LPR dispatch; C % 4 != 0 takes the scalar path.
HOP_CASES = [(1, 1, 0.0, (), 0), (1, 7, 0.6, (70,), 0), (2, 3, 0.5, (700,), 0), (8, 8, 0.6, (70, 1300), 0), (8, 8, 0.0, (), 0),
             (8, 64, 0.5, (65,), 2), (1, 128, 0.6, (), 0), (16, 5, 0.6, (70,), 1)]


def hop_inputs(H, C, long_rows, seed):
    """A random bipartite multigraph: 5 n_dst random edges from all n_src sources, 100 of them listed twice, the self-loop source t ->
    target t on every target, targets 0, 1, .. with rows of the given lengths; every source has at least one edge."""
    rng = np.random.default_rng(3000 * seed + 17 * H + C)
    src, dst = rng.integers(0, N_SRC, size=5 * N_DST), rng.integers(0, N_DST, size=5 * N_DST)
    src = np.concatenate([src, src[:100], np.arange(N_DST), np.arange(N_SRC)])
    dst = np.concatenate([dst, dst[:100], np.arange(N_DST), np.arange(N_SRC) % N_DST])
    for i, L in enumerate(long_rows):
        src, dst = np.concatenate([src, rng.integers(0, N_SRC, size=L)]), np.concatenate([dst, np.full(L, i)])
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    return (torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64)), f(N_SRC, H * C), f(N_SRC, H), f(N_DST, H),
            f(H * C), f(N_DST, H * C))


def _edge_keep(block, H, p, seed):
    """The hop's factors in edge-list order, through the library's keep-factor route (indexed by target-major slot)."""
    from allset_amd import dense
    k = dense.dropout_scale((block.nnz, H), p, seed, DEV)
    out = torch.empty_like(k)
    out[block.perm.long()] = k
    return out.cpu().double()


@pytest.mark.parametrize("case", HOP_CASES, ids=lambda c: f"H{c[0]}C{c[1]}-p{c[2]}-long{len(c[3])}")
def test_block_hop_vs_float64(monkeypatch, case):
    from allset_amd.functional import han_block_propagate
    from allset_amd.han_sampling import Block
    H, C, p, long_rows, seed = case
    src, dst, x, el, er, b, G = hop_inputs(H, C, long_rows, seed)
    block = Block.from_edges(src.to(DEV), dst.to(DEV), N_SRC, N_DST)
    seeds = _capture_seeds(monkeypatch)
    dv = [t.float().to(DEV).requires_grad_(True) for t in (x, el, er, b)]
    y = han_block_propagate(dv[0], dv[1], dv[2], block, H, 0.2, dv[3], p)
    assert tuple(y.shape) == (N_DST, H * C)
    (y * G.float().to(DEV)).sum().backward()
    keep = None
    if p > 0:
        assert len(seeds) == 1
        keep = _edge_keep(block, H, p, seeds[0])
        assert set(keep.unique().tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
    leaves = [t.clone().requires_grad_(True) for t in (x, el, er, b)]
    rep = []
    yo = orc.gat_hop(src, dst, N_SRC, N_DST, leaves[0], leaves[1], leaves[2], leaves[3], keep, rep)
    (yo * G).sum().backward()
    print(f"min |el[s] + er[t]| = {rep[0]:.3e}")
    assert rep[0] > sc.KINK_MARGIN
    _close(y, yo, "y")
    for got, want, what in zip(dv, leaves, ("gx", "gel", "ger", "gbias")):
        assert got.grad.shape == want.grad.shape
        _close(got.grad, want.grad, what)


def test_hop_cases_cover_the_kernel_paths():
    assert {c[0] for c in HOP_CASES} >= {1, 2, 8}
    assert any(c[0] * c[1] == 1 for c in HOP_CASES) and any(c[0] * c[1] == 512 for c in HOP_CASES)      # both dispatch extremes
    assert any(c[1] % 4 and c[0] * c[1] > 64 for c in HOP_CASES)
    assert any(c[3] and max(c[3]) > 1024 for c in HOP_CASES) and any(c[2] == 0.5 for c in HOP_CASES) and any(c[2] == 0.6 for c in HOP_CASES)


def test_square_block_is_bit_identical_to_the_full_batch_hop():
    from allset_amd.functional import han_block_propagate, han_gat_propagate
    from allset_amd.han import MetapathGraph
    from allset_amd.han_sampling import Block
    H, C, n = 8, 8, 700
    rng = np.random.default_rng(5)
    src = torch.from_numpy(np.concatenate([rng.integers(0, n, size=6 * n), np.arange(n)])).to(DEV)
    dst = torch.from_numpy(np.concatenate([rng.integers(0, n, size=6 * n), np.arange(n)])).to(DEV)
    graph, block = MetapathGraph(src, dst, n), Block.from_edges(src, dst, n, n)
    g = torch.Generator().manual_seed(0)
    ins = [torch.randn(*s, generator=g).to(DEV) for s in ((n, H * C), (n, H), (n, H), (H * C,), (n, H * C))]
    for p in (0.0, 0.6):
        res = []
        for fn, gr in ((han_gat_propagate, graph), (han_block_propagate, block)):
            torch.manual_seed(3)
            leaves = [t.clone().requires_grad_(True) for t in ins[:4]]
            y = fn(leaves[0], leaves[1], leaves[2], gr, H, 0.2, leaves[3], p)
            (y * ins[4]).sum().backward()
            res.append([y.detach()] + [t.grad for t in leaves])
        for a, b in zip(*res):
            assert torch.equal(a, b)


def test_stacked_write_over_a_non_square_block_equals_separate_calls_bitwise():
    """n_src = 5, n_dst = 3: the smallest shape at which a mix-up of the two row counts in the one autograd Function shows."""
    from allset_amd.functional import han_block_propagate
    from allset_amd.han_sampling import Block
    H, C, n_src, n_dst = 2, 4, 5, 3
    d = H * C
    edges = [([0, 1, 2, 3, 4], [0, 1, 2, 0, 1]), ([0, 1, 2, 3, 4, 4], [0, 1, 2, 2, 0, 1])]
    blks = [Block.from_edges(torch.tensor(s, device=DEV), torch.tensor(t, device=DEV), n_src, n_dst) for s, t in edges]
    g = torch.Generator().manual_seed(0)
    ins = [[torch.randn(*s, generator=g).to(DEV) for s in ((n_src, d), (n_src, H), (n_dst, H), (d,))] for _ in blks]
    G = torch.randn(n_dst, 2 * d, generator=g).to(DEV)

    def run(stacked):
        leaves = [[t.clone().requires_grad_(True) for t in one] for one in ins]
        if stacked:
            z = torch.full((n_dst, 2 * d), float("nan"), device=DEV)
            for i, (blk, (x, el, er, b)) in enumerate(zip(blks, leaves)):
                z = han_block_propagate(x, el, er, blk, H, 0.2, b, 0.0, out=z, block=i)
        else:
            z = torch.cat([han_block_propagate(x, el, er, blk, H, 0.2, b, 0.0) for blk, (x, el, er, b) in zip(blks, leaves)], dim=1)
        assert tuple(z.shape) == (n_dst, 2 * d)
        (z * G).sum().backward()
        return [z.detach()] + [t.grad for one in leaves for t in one]

    for a, b in zip(run(True), run(False)):
        assert torch.equal(a, b)


def test_unbuilt_shapes_and_bad_arguments_are_errors():
    from allset_amd import _lib, ops
    from allset_amd.functional import han_block_propagate
    from allset_amd.han_sampling import Block, HANSampler, DEFAULT_METAPATHS
    c, pairs, n_v, n_e, w = _walker()
    blk = Block.from_edges(torch.tensor([0, 1, 2, 3, 4], device=DEV), torch.tensor([0, 1, 2, 0, 1], device=DEV), 5, 3)
    z = lambda *s: torch.zeros(*s, device=DEV)
    with pytest.raises(_lib.AllSetHipError, match="exceeds the built maximum"):
        han_block_propagate(z(5, 1024), z(5, 2), z(3, 2), blk, 2)
    with pytest.raises(_lib.AllSetHipError, match="source"):
        han_block_propagate(z(4, 8), z(4, 2), z(3, 2), blk, 2)
    with pytest.raises(_lib.AllSetHipError, match="target"):
        han_block_propagate(z(5, 8), z(5, 2), z(5, 2), blk, 2)
    leaf = torch.zeros(3, 8, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="out must be a buffer"):
        han_block_propagate(z(5, 8), z(5, 2), z(3, 2), blk, 2, out=leaf * 1.0)
    with pytest.raises(ValueError, match="n_dst"):
        Block.from_edges(torch.tensor([0], device=DEV), torch.tensor([0], device=DEV), 2, 3)
    seeds32 = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.AllSetHipError, match="exceeds the built maximum"):
        ops.han_walk(0, w.v2e, w.e2v, 0, seeds32, 65, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="int32"):
        ops.han_walk(0, w.v2e, w.e2v, 0, seeds32.long(), 4, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="two orientations"):
        ops.han_walk(0, w.v2e, w.v2e, 0, seeds32, 4, 0, 0)
    with pytest.raises(ValueError, match="duplicate seeds"):
        HANSampler(w, DEFAULT_METAPATHS, 4).sample_blocks(torch.tensor([3, 5, 3], device=DEV))
    with pytest.raises(_lib.AllSetHipError):
        from allset_amd.han_sampling import MetapathWalker
        MetapathWalker(SimpleNamespace(edge_index=torch.from_numpy(pairs), n_x=[n_v], num_hyperedges=[n_e]))      # a CPU incidence
    # a device seed outside the node range is a node without out-edges: the self-loop alone, nothing read out of bounds
    _, blocks = HANSampler(w, DEFAULT_METAPATHS, 4).sample_blocks(torch.tensor([2, n_v + n_e + 5], device=DEV), counter=0)
    assert all(_rows(b)[n_v + n_e + 5] == [n_v + n_e + 5] for b in blocks)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _model_and_data(name):
    from allset_amd.han_sampling import Block, HAN
    c = sc.spec(name)
    x, pairs, n_v, n_e = sc.raw_data(c)
    blks = sc.blocks(c, pairs)
    dblocks = [Block.from_edges(b.src.to(DEV), b.dst.to(DEV), b.n_src, b.n_dst, b.src_ids.to(DEV)) for b in blks]
    torch.manual_seed(c["seed"])
    model = HAN(num_metapath=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=sc.DROPOUT)
    sd64 = sc.perturb(model.state_dict(), c)
    model.load_state_dict({k: v.float() for k, v in sd64.items()})
    sd64 = {k: v.detach().double() for k, v in model.state_dict().items()}               # the fp32 values the device model holds
    return c, model.to(DEV), blks, dblocks, x, sd64


MASK_SEED = {name: 1 for name in sc.CASES}


def _run_model(monkeypatch, name, training):
    from allset_amd import dense
    from allset_amd.han_sampling import load_subtensors
    c, model, blks, dblocks, x, sd64 = _model_and_data(name)
    H = c["heads"][0]
    model.train(training)
    seeds = _capture_seeds(monkeypatch)
    if training:
        torch.manual_seed(MASK_SEED[name])
    feats = torch.from_numpy(x).float().to(DEV)
    hd = [h.clone().requires_grad_(True) for h in load_subtensors(dblocks, feats)]
    logits = model(dblocks, hd)
    assert tuple(logits.shape) == (c["B"], c["C"])
    G = torch.from_numpy(sc.cotangent(c))
    (logits * G.float().to(DEV)).sum().backward()
    masks = None
    if training:
        assert len(seeds) == 4                                          # per conv: the feature mask, then the attention mask
        masks = []
        for i, (b, db) in enumerate(zip(blks, dblocks)):
            fk = dense.dropout_scale((b.n_src, c["F"]), sc.DROPOUT, seeds[2 * i], DEV).cpu().double()
            masks.append((fk, _edge_keep(db, H, sc.DROPOUT, seeds[2 * i + 1])))
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    ho = [torch.from_numpy(x).float().double()[b.src_ids].clone().requires_grad_(True) for b in blks]
    report = []
    lo = orc.han_forward(sd, blks, ho, masks, report)
    (lo * G).sum().backward()
    print(f"{name} training={training}: kink margin {min(report):.3e}")
    assert min(report) > sc.KINK_MARGIN
    _close(logits, lo, "logits")
    for i, (a, b) in enumerate(zip(hd, ho)):
        _close(a.grad, b.grad, f"grad_h{i}")
    for k, prm in model.named_parameters():
        _close(prm.grad, sd[k].grad, f"grad:{k}")
    return c, logits, hd, model


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_model_eval_vs_oracle_and_fixtures(monkeypatch, name):
    c, logits, hd, model = _run_model(monkeypatch, name, training=False)
    if not c["train"]:                                                  # the recorded reference ran this case in eval mode too
        fx = sc.load(sc.FILE)
        sc.assert_result(logits, fx, name, "out", **TOL)
        for i, h in enumerate(hd):
            sc.assert_result(h.grad, fx, name, f"grad_h{i}", **TOL)
        for k, prm in model.named_parameters():
            sc.assert_result(prm.grad, fx, name, f"grad:{k}", **TOL)


@pytest.mark.parametrize("name", sorted(n for n in sc.CASES if not n.startswith("cora")))
def test_model_training_vs_oracle_with_product_masks(monkeypatch, name):
    _run_model(monkeypatch, name, training=True)


def test_model_on_sampled_blocks_vs_oracle():
    """End to end on blocks the DEVICE sampler built (eval mode): sampler output -> model -> float64 restatement on the same blocks."""
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HAN, HANSampler, load_subtensors
    c, pairs, n_v, n_e, w = _walker("hs_h8")
    x, _, _, _ = sc.raw_data(c)
    seeds = sc.seed_nodes(c).tolist()
    _, dblocks = HANSampler(w, DEFAULT_METAPATHS, 6, seed=8).sample_blocks(seeds, counter=1)
    torch.manual_seed(c["seed"])
    model = HAN(num_metapath=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=sc.DROPOUT)
    model.load_state_dict({k: v.float() for k, v in sc.perturb(model.state_dict(), c).items()})
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    feats = torch.from_numpy(x).float().to(DEV)
    logits = model(dblocks, load_subtensors(dblocks, feats))
    blks = [SimpleNamespace(src=b.src.cpu(), dst=b.dst.cpu(), n_src=b.n_src, n_dst=b.n_dst, src_ids=b.src_ids.cpu()) for b in dblocks]
    report = []
    lo = orc.han_forward(sd, blks, [torch.from_numpy(x).float().double()[b.src_ids] for b in blks], None, report)
    assert min(report) > sc.KINK_MARGIN
    _close(logits, lo, "logits")


# ---- driver --------------------------------------------------------------------------------------------------------------------
DRIVER = ["--dataset", "synthetic", "--runs", "1", "--num_epochs", "4", "--batch_size", "64", "--lr", "0.005"]


def _drive():
    from allset_amd import han_sampling as hs
    return hs.main(hs.setup(hs.build_parser().parse_args(DRIVER).__dict__))


def test_driver_twice_is_bit_identical_and_lowers_the_training_loss(capsys):
    a = _drive()
    out = capsys.readouterr().out
    b = _drive()
    assert a["train_loss"] == b["train_loss"] and a["acc"] == b["acc"] and a["macro_f1"] == b["macro_f1"]
    losses = a["train_loss"][0]
    print(f"mean train loss per epoch: {['%.4f' % v for v in losses]}; test acc {a['acc'][0]:.2f}")
    assert len(losses) == 4 and losses[-1] < losses[0]
    assert ">> Final test acc:" in out and "test marco f1:" in out and ">> Train time per run:" in out
