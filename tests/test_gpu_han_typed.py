"""GPU: typed mini-batch HAN -- the L-hop metapath walk over a ``HeteroGraph`` (csrc/han_sample.hip ``allset_han_walk_typed``,
``han_sampling.TypedMetapathWalker``) on the tiny typed graph of tests/han_typed_cases.py: bit-identity with the two-hop walk for
L = 2, purity and batch independence, the endpoint distribution of 1-, 2-, 4- (one with a repeated relation) and 8-hop walks and
the collision rates against the float64 product of the row-stochastic relation matrices under the binomial 5-sigma bound,
termination (author-less papers, a dead intermediate node, out-of-range device seeds, an empty relation), the blocks against a numpy
restatement built from the raw endpoints, the model on typed blocks against the float64 restatement of tests/han_sampling_oracle.py
(its own criterion and kink margin), a training step, the ``--hetero`` driver twice, and the refusals."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_sampling_cases as sc  # noqa: E402
import han_sampling_oracle as orc  # noqa: E402
import han_typed_cases as tc  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = dict(rtol=1e-4, atol=1e-4)                  # tests/test_gpu_han_sampling.py's criterion for this model
DEV = torch.device("cuda:0")
PAP_PFP = [["pa", "ap"], ["pf", "fp"]]


@pytest.fixture(scope="module")
def g():
    return tc.hetero_graph(DEV)


def _walker(g):
    from allset_amd.han_sampling import TypedMetapathWalker
    return TypedMetapathWalker(g)


def _i32(ids):
    return torch.tensor(ids, dtype=torch.int32, device=DEV)


def _rows(block):
    """{global target id: [global source ids in slot order]} of a sampled block."""
    rp, col, ids = block.rowptr.cpu().numpy(), block.col.cpu().numpy(), block.src_ids.cpu().numpy()
    return {int(ids[t]): [int(ids[s]) for s in col[rp[t]:rp[t + 1]]] for t in range(block.n_dst)}


# ---- 1. L = 2 is the shipped walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,k", [(1, 1), (5, 7), (58, 64)])
@pytest.mark.parametrize("m", [0, 1])
def test_two_hops_are_bit_identical_to_the_shipped_walk(m, B, k):
    from allset_amd import ops
    from allset_amd.han_sampling import MetapathWalker
    c = sc.spec("hs_h2")
    _, pairs, n_v, n_e = sc.raw_data(c)
    w = MetapathWalker(SimpleNamespace(edge_index=torch.from_numpy(pairs).to(DEV), n_x=[n_v], num_hyperedges=[n_e]))
    seeds = _i32(np.random.default_rng(B).permutation(n_v + n_e)[:B].tolist())   # vertices, isolated ones, ids past the rows
    for seed, ctr in ((7, 3), (2 ** 40 + 1, 2 ** 33)):
        want = ops.han_walk(m, w.v2e, w.e2v, 0, seeds, k, seed, ctr)
        got = ops.han_walk_typed(m, [w.v2e, w.e2v], seeds, k, seed, ctr)
        assert got.dtype == torch.int32 and tuple(got.shape) == (B, k) and torch.equal(got, want)
    if B > 1:
        assert int((want >= 0).sum()) > 0 and int((want < 0).sum()) > 0           # both walked and terminated lanes were compared


# ---- 2. purity ----------------------------------------------------------------------------------------------------------------------
def test_equal_arguments_give_equal_bits_and_a_row_does_not_depend_on_the_batch(g):
    from allset_amd.han_sampling import random_walk_endpoints
    w = _walker(g)
    mp = tc.METAPATHS["papfp"]
    seeds = [3, 17, 5, 38, 20, 1]
    a = random_walk_endpoints(w, mp, seeds, 16, 4, 9)
    assert a.dtype == torch.int64 and tuple(a.shape) == (6, 16)
    assert torch.equal(a, random_walk_endpoints(w, mp, torch.tensor(seeds, device=DEV), 16, 4, 9))
    assert not torch.equal(a, random_walk_endpoints(w, mp, seeds, 16, 4, 10))                 # another counter
    assert not torch.equal(a, random_walk_endpoints(w, mp, seeds, 16, 5, 9))                  # another seed
    assert not torch.equal(a, random_walk_endpoints(w, mp, seeds, 16, 4, 9, index=1))         # another metapath index
    other = [38, 30, 5, 9, 3, 11, 12, 13, 14]
    many = list(range(39, -1, -1))                                                           # 40 x 16 lanes: three blocks
    b, c = random_walk_endpoints(w, mp, other, 16, 4, 9), random_walk_endpoints(w, mp, many, 16, 4, 9)
    for node in (3, 5, 38):
        assert torch.equal(a[seeds.index(node)], b[other.index(node)]) and torch.equal(a[seeds.index(node)], c[many.index(node)])
    assert torch.equal(a[0], random_walk_endpoints(w, mp, [3], 16, 4, 9)[0])                  # alone


# ---- 3. distribution ------------------------------------------------------------------------------------------------------------------
DIST_SEEDS = {"pap": [0, 1, 7, 19, 37, 38], "papfp": [0, 3, 12, 39], "papap": [0, 5, 21, 33], "cites": [0, 2, 17, 29, 31],
              "hop8": [1, 20]}


@pytest.mark.parametrize("name", sorted(DIST_SEEDS))
def test_walk_endpoints_follow_the_exact_distribution_and_hops_and_lanes_are_independent(g, name):
    """k = 64 walks over 256 counters = 16384 walks per seed, seed 12345 (fixed before the first run), 5-sigma binomial bounds."""
    from allset_amd.han_sampling import random_walk_endpoints
    w = _walker(g)
    mp, seeds = tc.METAPATHS[name], DIST_SEEDS[name]
    k, counters = 64, 256
    walks = torch.stack([random_walk_endpoints(w, mp, seeds, k, 12345, ctr) for ctr in range(counters)]).cpu().numpy()
    assert walks.shape == (counters, len(seeds), k)
    for i, s in enumerate(seeds):
        tc.check_walks(walks[:, i, :], tc.endpoint_law(mp, s), f"{name} seed {s}")


# ---- 4. termination -----------------------------------------------------------------------------------------------------------------
def test_walks_terminate_with_minus_one_and_read_nothing_out_of_range(g):
    from allset_amd.han_sampling import HANSampler, random_walk_endpoints
    w = _walker(g)
    ends = random_walk_endpoints(w, ["pa", "ap"], list(tc.ORPHANS) + [0], 64, 1, 0)
    assert bool((ends[:2] == -1).all()) and bool((ends[2] >= 0).all())
    _, blocks = HANSampler(w, PAP_PFP, 8, seed=3).sample_blocks([4, tc.ORPHANS[0], 9, tc.ORPHANS[1]], counter=2)
    rows = _rows(blocks[0])
    assert rows[tc.ORPHANS[0]] == [tc.ORPHANS[0]] and rows[tc.ORPHANS[1]] == [tc.ORPHANS[1]] and len(rows[4]) > 1
    assert all(len(r) > 1 for r in _rows(blocks[1]).values())                                # every paper has a field
    # the r1, r2 chain: -1 exactly for the walks that reach the b node without an out-edge
    wa = _walker(g)
    seeds = [1, 4, 9, 14, 0]
    walks = torch.stack([random_walk_endpoints(wa, tc.METAPATHS["r1r2"], seeds, 64, 12345, ctr) for ctr in range(256)]).cpu().numpy()
    for i, s in enumerate(seeds):
        law = tc.endpoint_law(tc.METAPATHS["r1r2"], s)
        r1 = tc.counts("r1")[s]
        assert law.get(-1, 0.0) == pytest.approx(r1[tc.DEAD_B] / r1.sum(), abs=1e-15)         # the exact probability of the dead node
        tc.check_walks(walks[:, i, :], law, f"r1r2 seed {s}")                                # ... -1's frequency among the endpoints
    assert tc.endpoint_law(tc.METAPATHS["r1r2"], 1)[-1] == 0.5 and -1 not in tc.endpoint_law(tc.METAPATHS["r1r2"], 0)
    # a device-resident seed tensor is taken as it is: ids outside the type's range have no out-edge
    dev_seeds = torch.tensor([2, tc.N["p"], tc.N["p"] + 5, 10 ** 6, -7, 2 ** 31 - 1], device=DEV)
    ends = random_walk_endpoints(w, tc.METAPATHS["papfp"], dev_seeds, 32, 1, 0)
    assert bool((ends[1:] == -1).all()) and bool((ends[0] >= 0).all())
    _, blocks = HANSampler(w, PAP_PFP, 4).sample_blocks(torch.tensor([2, tc.N["p"] + 5], device=DEV), counter=0)
    assert all(_rows(b)[tc.N["p"] + 5] == [tc.N["p"] + 5] for b in blocks)
    # a relation without edges: every walk terminates, alone and in the middle of a chain
    assert bool((random_walk_endpoints(w, ["e0"], list(range(40)), 8, 1, 0) == -1).all())
    assert bool((random_walk_endpoints(w, ["cites", "e0", "cites"], list(range(40)), 8, 1, 0) == -1).all())


# ---- 5. blocks ----------------------------------------------------------------------------------------------------------------------
def test_blocks_equal_the_numpy_restatement_built_from_the_raw_endpoints(g):
    from allset_amd.han_sampling import HANSampler, load_subtensors, random_walk_endpoints
    w = _walker(g)
    seeds = np.random.default_rng(1).permutation(tc.N["p"])[:23].tolist()
    assert set(tc.ORPHANS) & set(seeds)
    k, seed, ctr = 9, 11, 5
    got_seeds, blocks = HANSampler(w, PAP_PFP, k, seed=seed).sample_blocks(seeds, counter=ctr)
    assert list(got_seeds) == seeds and len(blocks) == 2
    feats = load_subtensors(blocks, torch.arange(tc.N["p"], device=DEV).float().view(-1, 1))
    B = len(seeds)
    for i, (mp, b) in enumerate(zip(PAP_PFP, blocks)):
        ends = random_walk_endpoints(w, mp, seeds, k, seed, ctr, index=i).cpu().numpy()
        rows = [sorted(set(ends[j].tolist()) - {-1, s}) + [s] for j, s in enumerate(seeds)]   # distinct, ascending, one self-loop last
        src_ids, src, dst, n_src, n_dst = orc.to_block(rows, seeds)                          # seeds first, then the others ascending
        assert (b.n_src, b.n_dst, b.nnz) == (n_src, n_dst, src.size)
        assert np.array_equal(b.src_ids.cpu().numpy(), src_ids)
        assert np.array_equal(feats[i].cpu().numpy()[:, 0], src_ids.astype(np.float32))
        assert _rows(b) == {s: r for s, r in zip(seeds, rows)}
        assert np.array_equal(b.col.cpu().numpy(), src) and np.array_equal(b.dst.cpu().numpy(), dst)   # target-major = the edge list
        assert np.array_equal(b.src.cpu().numpy(), src)
        rp, perm = b.rowptr.cpu().numpy(), b.perm.cpu().numpy()
        assert np.array_equal(rp, np.concatenate([[0], np.cumsum([len(r) for r in rows])])) and np.array_equal(perm, np.arange(src.size))
        rpT, colT, slotT = b.rowptrT.cpu().numpy(), b.colT.cpu().numpy(), b.slotT.cpu().numpy()
        assert rpT.size == n_src + 1 and rpT[0] == 0 and rpT[-1] == src.size
        assert sorted(slotT.tolist()) == list(range(src.size))
        assert np.array_equal(src[slotT], np.repeat(np.arange(n_src), np.diff(rpT))) and np.array_equal(dst[slotT], colT)
    assert any(len(r) > 1 for r in _rows(blocks[0]).values())
    with pytest.raises(ValueError, match="duplicate seeds"):
        HANSampler(w, PAP_PFP, 4).sample_blocks(torch.tensor([3, 5, 3], device=DEV))
    with pytest.raises(ValueError, match="duplicate seeds"):
        HANSampler(w, PAP_PFP, 4).sample_blocks([3, 5, 3])
    with pytest.raises(ValueError, match="outside"):
        HANSampler(w, PAP_PFP, 4).sample_blocks([3, tc.N["p"]])                               # host seeds: checked against walker.n
    assert w.ntype == "p" and w.n == tc.N["p"]


# ---- 6. model -----------------------------------------------------------------------------------------------------------------------
def _model(c):
    from allset_amd.han_sampling import HAN
    torch.manual_seed(c["seed"])
    model = HAN(num_metapath=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=sc.DROPOUT)
    model.load_state_dict({k: v.float() for k, v in sc.perturb(model.state_dict(), c).items()})
    return model


def test_model_on_typed_blocks_vs_oracle(g):
    """End to end on blocks the typed sampler built (eval mode): sampler output -> model -> float64 restatement on the same blocks."""
    from allset_amd.han_sampling import HANSampler, load_subtensors
    c = sc.spec("hs_h8")
    x = sc.raw_data(c)[0][:tc.N["p"]]                                             # the case's feature rows of its 40 vertices
    seeds = [0, 7, 12, 38, 3, 25, 31, 39, 16, 9]
    _, dblocks = HANSampler(_walker(g), PAP_PFP, 6, seed=8).sample_blocks(seeds, counter=1)
    model = _model(c)
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    model = model.to(DEV).eval()
    feats = torch.from_numpy(x).float().to(DEV)
    logits = model(dblocks, load_subtensors(dblocks, feats))
    blks = [SimpleNamespace(src=b.src.cpu(), dst=b.dst.cpu(), n_src=b.n_src, n_dst=b.n_dst, src_ids=b.src_ids.cpu()) for b in dblocks]
    report = []
    lo = orc.han_forward(sd, blks, [torch.from_numpy(x).float().double()[b.src_ids] for b in blks], None, report)
    print(f"kink margin {min(report):.3e}; max |diff| {float((logits.detach().cpu().double() - lo).abs().max()):.3e}")
    assert min(report) > sc.KINK_MARGIN
    torch.testing.assert_close(logits.detach().cpu().double(), lo.detach(), **TOL)


def test_training_step_on_typed_blocks_has_gradients_and_is_bit_stable(g):
    from allset_amd.han_sampling import HANSampler, load_subtensors
    c = sc.spec("hs_h8")
    feats = torch.from_numpy(sc.raw_data(c)[0][:tc.N["p"]]).float().to(DEV)
    seeds = list(range(0, 40, 2))
    labels = torch.arange(len(seeds), device=DEV) % c["C"]

    def run():
        model = _model(c).to(DEV).train()
        torch.manual_seed(5)
        _, blocks = HANSampler(_walker(g), PAP_PFP, 6, seed=8).sample_blocks(seeds, counter=1)
        loss = torch.nn.functional.cross_entropy(model(blocks, load_subtensors(blocks, feats)), labels)
        loss.backward()
        return [loss.detach()] + [p.grad for _, p in model.named_parameters()], [n for n, _ in model.named_parameters()]

    (a, names), (b, _) = run(), run()
    for name, x, y in zip(["loss"] + names, a, b):
        assert bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0, name
        assert torch.equal(x, y), name


# ---- 7. driver ----------------------------------------------------------------------------------------------------------------------
DRIVER = ["--hetero", "--dataset", "synthetic", "--runs", "1", "--num_epochs", "4", "--batch_size", "64", "--lr", "0.005"]


def _drive(argv=DRIVER):
    from allset_amd import han_sampling as hs
    return hs.main(hs.setup(hs.build_parser().parse_args(argv).__dict__))


def test_hetero_driver_twice_is_bit_identical_and_lowers_the_training_loss(capsys):
    a = _drive()
    out = capsys.readouterr().out
    b = _drive()
    assert a["train_loss"] == b["train_loss"] and a["acc"] == b["acc"] and a["macro_f1"] == b["macro_f1"]
    losses = a["train_loss"][0]
    print(f"mean train loss per epoch: {['%.4f' % v for v in losses]}; test acc {a['acc'][0]:.2f}")
    assert len(losses) == 4 and losses[-1] < losses[0]
    assert ">> Final test acc:" in out and "test marco f1:" in out and ">> Train time per run:" in out
    with pytest.raises(FileNotFoundError, match="not available to --hetero"):
        _drive(["--hetero", "--dataset", "cora", "--runs", "1", "--num_epochs", "1"])


# ---- 8. refusals ----------------------------------------------------------------------------------------------------------------------
def test_unbuilt_lengths_and_bad_arguments_are_errors(g):
    from allset_amd import _lib, ops
    pa, ap, pf = g.csr("pa"), g.csr("ap"), g.csr("pf")
    seeds = _i32([0, 1])
    assert ops.HAN_MAX_HOPS == 8
    assert tuple(ops.han_walk_typed(0, [pa, ap] * 4, seeds, 4, 0, 0).shape) == (2, 4)           # the cap itself is built
    with pytest.raises(_lib.AllSetHipError, match="HAN_MAX_HOPS = 8"):
        ops.han_walk_typed(0, [pa, ap] * 4 + [pa], seeds, 4, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="HAN_MAX_HOPS = 8"):
        ops.han_walk_typed(0, [], seeds, 4, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="exceeds the built maximum"):
        ops.han_walk_typed(0, [pa, ap], seeds, 65, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="k >= 1"):
        ops.han_walk_typed(0, [pa, ap], seeds, 0, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="int32"):
        ops.han_walk_typed(0, [pa, ap], seeds.long(), 4, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="do not meet"):
        ops.han_walk_typed(0, [pa, pf], seeds, 4, 0, 0)
    with pytest.raises(_lib.AllSetHipError, match="metapath index"):
        ops.han_walk_typed(256, [pa, ap], seeds, 4, 0, 0)
    with pytest.raises(_lib.AllSetHipError):
        ops.han_walk_typed(0, [pa, ap], seeds.cpu(), 4, 0, 0)                                  # no fallback for host tensors
