"""GPU: the sync-free fixed-capacity block path of mini-batch HAN (csrc/han_sample.hip ``allset_han_walk_dc`` /
``allset_han_walk_typed_dc`` / ``allset_han_block_relabel`` / ``_compact_fixed`` / ``_transpose``; han_sampling ``FixedBlock``,
``HANSampler.sample_blocks_fixed``, ``GraphedSampledStep``, ``--fixed_blocks`` / ``--graph_step``): the device step counter against the
by-value walks, the fixed blocks entry for entry against ``sample_blocks``, the padding contract, capture of the sampler alone, the
model on padded blocks against the float64 restatement and against the exact block, and the graphed step against the eager one.

The relabel kernel loops by chunks of 1024 entries (``kScanBlock``) over the B counts and over the B (k + 1) slab entries; the shapes
below stand on each side of that width for both loops.  The transpose kernel has no chunk loop (one lane per source row)."""
from __future__ import annotations

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
M64 = (1 << 64) - 1


def _close(got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    print(f"{what}: max |diff| {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got, want, msg=lambda m: f"{what}: {m}", **TOL)


_WALKERS = {}


def _walker(name="hs_h2"):
    from allset_amd.han_sampling import MetapathWalker
    if name not in _WALKERS:
        c = sc.spec(name)
        _, pairs, n_v, n_e = sc.raw_data(c)
        data = SimpleNamespace(edge_index=torch.from_numpy(pairs).to(DEV), n_x=[n_v], num_hyperedges=[n_e])
        _WALKERS[name] = (c, n_v, n_e, MetapathWalker(data))
    return _WALKERS[name]


@pytest.fixture(scope="module")
def g():
    return tc.hetero_graph(DEV)


def _i32(ids):
    return torch.tensor(np.asarray(ids), dtype=torch.int32, device=DEV)


def _counter_tensor(c):
    """One int64 device element with the 64 bits of ``c``."""
    return torch.tensor([c - (1 << 64) if c >= (1 << 63) else c], dtype=torch.int64, device=DEV)


# ---- 1. the device step counter ------------------------------------------------------------------------------------------------
COUNTERS = [(0, 0), (9, 0), (2 ** 32 + 5, 0), (7, 1 << 40), (2 ** 64 - 1, 2)]        # the last one wraps


@pytest.mark.parametrize("m", [0, 1])
def test_device_counter_two_hop_walk_is_bit_identical(m):
    from allset_amd import ops
    c, n_v, n_e, w = _walker()
    a, b, base = w.orientation(m)
    seeds = _i32(np.random.default_rng(3).permutation(n_v + n_e)[:37])
    outs = []
    for cv, add in COUNTERS:
        want = ops.han_walk(m, a, b, base, seeds, 7, 11, (cv + add) & M64)
        got = ops.han_walk(m, a, b, base, seeds, 7, 11, _counter_tensor(cv), counter_add=add)
        assert got.dtype == torch.int32 and torch.equal(got, want)
        assert torch.equal(ops.han_walk(m, a, b, base, seeds, 7, 11, cv, counter_add=add), want)      # an int counter adds on the host
        outs.append(want)
    assert int((outs[0] >= 0).sum()) > 0 and not torch.equal(outs[0], outs[1])
    if hasattr(torch, "uint64"):
        u = torch.tensor([9], dtype=torch.int64, device=DEV).view(torch.uint64)
        assert torch.equal(ops.han_walk(m, a, b, base, seeds, 7, 11, u), outs[1])


@pytest.mark.parametrize("hops", [1, 2, 8])
def test_device_counter_typed_walk_is_bit_identical(g, hops):
    from allset_amd import ops
    chain = {1: tc.METAPATHS["cites"], 2: tc.METAPATHS["pap"], 8: tc.METAPATHS["hop8"]}[hops]
    csrs = [g.csr(e) for e in chain]
    seeds = _i32(np.random.default_rng(4).permutation(tc.N["p"] + 3)[:29])           # ids past the rows too
    outs = []
    for cv, add in COUNTERS:
        want = ops.han_walk_typed(2, csrs, seeds, 9, 5, (cv + add) & M64)
        got = ops.han_walk_typed(2, csrs, seeds, 9, 5, _counter_tensor(cv), counter_add=add)
        assert torch.equal(got, want)
        outs.append(want)
    assert int((outs[0] >= 0).sum()) > 0 and not torch.equal(outs[0], outs[2])


# ---- 2. block identity and the padding contract ---------------------------------------------------------------------------------
def _check_fixed(fb, blk, k, seeds, what):
    """``fb`` (FixedBlock) against the eager ``blk`` for the same inputs: sizes, the real part entry for entry, the padding contract."""
    from allset_amd.han_sampling import FixedBlock
    B, nnz, n_src = blk.n_dst, blk.nnz, blk.n_src
    cap = B * (k + 1)
    assert isinstance(fb, FixedBlock) and (fb.n_dst, fb.n_src, fb.nnz) == (B, cap, cap), what
    assert fb.sizes.dtype == torch.int32 and fb.sizes.tolist() == [nnz, n_src - B], what
    assert [t.numel() for t in (fb.rowptr, fb.col, fb.dst32, fb.src_ids, fb.rowptrT, fb.colT, fb.slotT)] == \
        [B + 1, cap, cap, cap, cap + 1, cap, cap], what
    assert fb.src_ids.dtype == torch.int64 and all(t.dtype == torch.int32 for t in (fb.rowptr, fb.col, fb.dst32, fb.rowptrT, fb.colT, fb.slotT))
    # content
    assert torch.equal(fb.rowptr, blk.rowptr) and int(fb.rowptr[B]) == nnz, what
    assert torch.equal(fb.col[:nnz], blk.col) and torch.equal(fb.dst[:nnz], blk.dst) and torch.equal(fb.src[:nnz], blk.src), what
    assert torch.equal(fb.src_ids[:n_src], blk.src_ids), what
    assert torch.equal(fb.rowptrT[:n_src + 1], blk.rowptrT) and torch.equal(fb.colT[:nnz], blk.colT), what
    assert torch.equal(fb.slotT[:nnz], blk.slotT) and torch.equal(fb.perm[:nnz], blk.perm), what
    # padding: empty source rows, every index in range over the full capacity
    assert bool((fb.rowptrT[n_src:] == nnz).all()), what
    for t, hi in ((fb.col, cap), (fb.colT, B), (fb.dst32, B), (fb.slotT, cap)):
        assert int(t.min()) >= 0 and int(t.max()) < hi, what
    assert int(fb.col[:nnz].max()) < n_src
    assert bool((fb.src_ids[n_src:] == int(seeds[0])).all()), what
    for t in (fb.col[nnz:], fb.colT[nnz:], fb.dst32[nnz:], fb.slotT[nnz:]):
        assert not t.numel() or int(t.abs().max()) == 0, what
    ex = fb.exact()
    assert (ex.n_dst, ex.n_src, ex.nnz) == (B, n_src, nnz)
    for a, b in zip((ex.src_ids, ex.src, ex.dst, ex.rowptr, ex.col, ex.perm, ex.rowptrT, ex.colT, ex.slotT),
                    (blk.src_ids, blk.src, blk.dst, blk.rowptr, blk.col, blk.perm, blk.rowptrT, blk.colT, blk.slotT)):
        assert torch.equal(a, b), what


def _both(sampler_args, seeds, counter):
    """The eager and the fixed blocks of one (seed, counter, seeds); ``seeds`` a device tensor (taken as it is: ids past the graph
    are nodes without out-edges)."""
    from allset_amd.han_sampling import HANSampler
    eager = HANSampler(*sampler_args).sample_blocks(seeds, counter=counter)[1]
    s = HANSampler(*sampler_args)
    fixed = s.sample_blocks_fixed(seeds, counter=counter)[1]
    s.check()
    return eager, fixed


# (B, k): the issue's shapes; slabs of 1023 / 1024 / 1025 = one side and the other of the relabel kernel's chunk over the slab;
# B = 1023 / 1024 / 1025 the same for its chunk over the counts (B = 1025, k = 1 also runs three slab chunks)
SHAPES = [(1, 1), (3, 2), (6, 8), (5, 64), (31, 32), (32, 31), (41, 24), (1023, 1), (1024, 1), (1025, 1)]


@pytest.mark.parametrize("B,k", SHAPES)
def test_fixed_blocks_equal_the_eager_blocks_hypergraph(B, k):
    from allset_amd.han_sampling import DEFAULT_METAPATHS
    c, n_v, n_e, w = _walker()
    n = n_v + n_e
    seeds = _i32(np.random.default_rng(B * 100 + k).permutation(max(n, B + 7))[:B])   # vertices, isolated ones, hyperedge nodes, ids past n
    eager, fixed = _both((w, DEFAULT_METAPATHS, k, 5), seeds, 3)
    assert len(fixed) == 2
    for mp, (fb, blk) in enumerate(zip(fixed, eager)):
        _check_fixed(fb, blk, k, seeds, f"B={B} k={k} metapath {mp}")
    if 31 <= B < n:
        assert eager[0].n_src > B and eager[0].nnz > B                               # the case has neighbours and non-seed sources
    if B > n:
        assert eager[0].n_src == B and eager[0].nnz > B                              # every node is a seed: neighbours, no other source


@pytest.mark.parametrize("B,k", SHAPES)
def test_fixed_blocks_equal_the_eager_blocks_typed(g, B, k):
    from allset_amd.han_sampling import TypedMetapathWalker
    w = TypedMetapathWalker(g)
    seeds = _i32(np.random.default_rng(B * 100 + k + 1).permutation(max(tc.N["p"], B + 5))[:B])
    eager, fixed = _both((w, [tc.METAPATHS["papfp"]], k, 9), seeds, 2 ** 33 + 1)
    _check_fixed(fixed[0], eager[0], k, seeds, f"typed B={B} k={k}")


@pytest.mark.parametrize("B,k", [(300, 20), (1024, 20)])
def test_fixed_blocks_equal_the_eager_blocks_many_distinct_sources(B, k):
    """Cora-shaped: thousands of real entries in the sorted extra slab, so the compaction of the distinct ids crosses many chunks."""
    from allset_amd.han_sampling import DEFAULT_METAPATHS
    c, n_v, n_e, w = _walker("cora_hs")
    seeds = _i32(np.random.default_rng(B).choice(n_v + n_e, size=B, replace=False))
    eager, fixed = _both((w, DEFAULT_METAPATHS, k, 1), seeds, 0)
    for mp, (fb, blk) in enumerate(zip(fixed, eager)):
        _check_fixed(fb, blk, k, seeds, f"cora B={B} k={k} metapath {mp}")
    assert int((eager[0].col >= B).sum()) > 1024                                      # real entries of the extra slab past one chunk
    if B == 1024:
        assert eager[0].n_src - B > 1024                                             # and distinct ones past one chunk of uniq


def test_fixed_blocks_special_seed_sets():
    from allset_amd.han_sampling import DEFAULT_METAPATHS, MetapathWalker
    c, n_v, n_e, w = _walker()
    # an isolated vertex: its row is the self-loop only
    seeds = _i32([n_v - 1, 3, 17])
    eager, fixed = _both((w, DEFAULT_METAPATHS, 6, 2), seeds, 1)
    assert int(eager[0].rowptr[1]) == 1 and int(eager[0].col[0]) == 0
    for fb, blk in zip(fixed, eager):
        _check_fixed(fb, blk, 6, seeds, "isolated vertex")
    # hyperedge-node seeds on VEV: every walk terminates
    seeds = _i32([n_v + 2, n_v, n_v + 7, n_v + 5])
    eager, fixed = _both((w, DEFAULT_METAPATHS, 6, 2), seeds, 1)
    assert eager[0].nnz == 4 and eager[0].n_src == 4 and eager[1].nnz > 4
    for fb, blk in zip(fixed, eager):
        _check_fixed(fb, blk, 6, seeds, "hyperedge-node seeds")
    assert fixed[0].sizes.tolist() == [4, 0]
    # every endpoint is itself a seed: all vertices are seeds
    seeds = _i32(np.random.default_rng(0).permutation(n_v))
    eager, fixed = _both((w, DEFAULT_METAPATHS, 6, 2), seeds, 1)
    assert eager[0].n_src == n_v and eager[0].nnz > n_v
    _check_fixed(fixed[0], eager[0], 6, seeds, "every endpoint a seed")
    assert fixed[0].sizes.tolist() == [eager[0].nnz, 0]
    # a batch inside one hub hyperedge with a single outside member
    pairs = np.array([[0, 1, 2, 3, 4, 5], [0, 0, 0, 0, 0, 1]])
    hub = MetapathWalker(SimpleNamespace(edge_index=torch.from_numpy(pairs).to(DEV), n_x=[6], num_hyperedges=[2]))
    seeds = _i32([2, 0, 3, 1])
    eager, fixed = _both((hub, DEFAULT_METAPATHS, 16, 2), seeds, 1)
    assert eager[0].n_src == 5 and int(eager[0].src_ids[4]) == 4
    _check_fixed(fixed[0], eager[0], 16, seeds, "hub hyperedge")
    assert fixed[0].sizes.tolist()[1] == 1


# ---- 3. capture: no synchronisation, fixed shapes -------------------------------------------------------------------------------
def test_sampler_alone_is_capturable_and_duplicates_reach_check():
    from allset_amd.graphs import GraphedCallable
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HANSampler
    c, n_v, n_e, w = _walker()
    B, k = 9, 5
    s = HANSampler(w, DEFAULT_METAPATHS, k, seed=6)
    buf = _i32(np.arange(B))
    ctr = torch.zeros(1, dtype=torch.int64, device=DEV)
    held = {}

    def fn():
        held["blocks"] = s.sample_blocks_fixed(buf, counter=ctr, counter_add=100)[1]
        return held["blocks"][0].sizes

    gc = GraphedCallable(fn, DEV)
    blocks = held["blocks"]                                                           # the static outputs of the captured graph
    rng = np.random.default_rng(8)
    for cv in (0, 4, 2 ** 35):
        ids = rng.permutation(n_v + n_e)[:B]
        buf.copy_(_i32(ids))
        ctr.fill_(cv)
        sizes = gc()
        eager = HANSampler(w, DEFAULT_METAPATHS, k, seed=6).sample_blocks(ids.tolist(), counter=cv + 100)[1]
        assert sizes.tolist() == [eager[0].nnz, eager[0].n_src - B]
        for mp, (fb, blk) in enumerate(zip(blocks, eager)):
            _check_fixed(fb, blk, k, ids, f"replay counter {cv} metapath {mp}")
    s.check()                                                                         # no duplicates so far
    ids = rng.permutation(n_v)[:B]
    ids[4] = ids[1]
    buf.copy_(_i32(ids))
    gc()
    buf.copy_(_i32(rng.permutation(n_v)[:B]))
    gc()                                                                              # sticky: a clean batch afterwards does not clear it
    with pytest.raises(ValueError, match="duplicate seeds"):
        s.check()
    s.check()                                                                         # reading it cleared it
    with pytest.raises(ValueError, match="duplicate seeds"):                          # a host list is checked on the host, as before
        s.sample_blocks_fixed([1, 2, 1])


# ---- 4. the model on padded blocks ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("name", ["hs_h1", "hs_h8"])
def test_model_on_fixed_blocks_vs_oracle_and_exact_blocks(name, training):
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HAN, HANSampler, load_subtensors
    c, n_v, n_e, w = _walker(name)
    x, _, _, _ = sc.raw_data(c)
    seeds = sc.seed_nodes(c).tolist()                                                 # vertices, an isolated one, a hyperedge node
    B, k = len(seeds), 6
    _, fixed = HANSampler(w, DEFAULT_METAPATHS, k, seed=8).sample_blocks_fixed(seeds, counter=1)
    exact = [fb.exact() for fb in fixed]
    assert any(e.n_src < fb.n_src for e, fb in zip(exact, fixed))
    torch.manual_seed(c["seed"])
    model = HAN(num_metapath=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=0.0)
    model.load_state_dict({k_: v.float() for k_, v in sc.perturb(model.state_dict(), c).items()})
    sd = {k_: v.detach().double().clone().requires_grad_(True) for k_, v in model.state_dict().items()}
    model = model.to(DEV).train(training)
    feats = torch.from_numpy(x).float().to(DEV)
    G = torch.from_numpy(sc.cotangent(c))

    def run(blocks):
        model.zero_grad(set_to_none=True)
        hd = [h.clone().requires_grad_(True) for h in load_subtensors(blocks, feats)]
        logits = model(blocks, hd)
        (logits * G.float().to(DEV)).sum().backward()
        return logits.detach(), [h.grad for h in hd], {k_: p.grad.clone() for k_, p in model.named_parameters()}

    lf, hf, gf = run(fixed)
    le, he, ge = run(exact)
    blks = [SimpleNamespace(src=b.src.cpu(), dst=b.dst.cpu(), n_src=b.n_src, n_dst=b.n_dst, src_ids=b.src_ids.cpu()) for b in exact]
    ho = [torch.from_numpy(x).float().double()[b.src_ids].clone().requires_grad_(True) for b in blks]
    report = []
    lo = orc.han_forward(sd, blks, ho, None, report)
    (lo * G).sum().backward()
    print(f"{name} training={training}: kink margin {min(report):.3e}")
    assert min(report) > sc.KINK_MARGIN
    assert tuple(lf.shape) == (B, c["C"])
    _close(lf, lo, "logits vs oracle")
    _close(lf, le, "logits vs exact block")
    for i, (e, fb) in enumerate(zip(exact, fixed)):
        assert tuple(hf[i].shape) == (fb.n_src, c["F"])
        _close(hf[i][:e.n_src], ho[i].grad, f"grad_h{i} vs oracle")
        _close(hf[i][:e.n_src], he[i], f"grad_h{i} vs exact block")
        assert int((hf[i][e.n_src:] != 0).sum()) == 0                                 # padded source rows: exact zeros
    for k_ in gf:
        _close(gf[k_], sd[k_].grad, f"grad:{k_} vs oracle")
        _close(gf[k_], ge[k_], f"grad:{k_} vs exact block")


# ---- 5. the graphed step --------------------------------------------------------------------------------------------------------
def _training_setup(dropout, seed=3):
    from allset_amd.han_sampling import DEFAULT_METAPATHS, HAN, HANSampler
    from allset_amd.optim import FusedAdam
    c, n_v, n_e, w = _walker("hs_h8")
    x, _, _, _ = sc.raw_data(c)
    feats = torch.from_numpy(x).float().to(DEV)
    labels = torch.from_numpy(np.random.default_rng(1).integers(0, c["C"], size=n_v + n_e)).to(DEV)
    torch.manual_seed(seed)
    model = HAN(num_metapath=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=dropout).to(DEV)
    sampler = HANSampler(w, DEFAULT_METAPATHS, 5, seed=4)
    opt = FusedAdam(model.parameters(), lr=0.01, weight_decay=0.001)
    return model, sampler, feats, labels, opt, n_v


def test_graphed_step_equals_the_eager_fixed_step_bit_for_bit():
    """Dropout 0: five replayed steps against five eager steps over ``sample_blocks_fixed`` from the same state and batches; the
    losses and every parameter bit-identical (same kernels, same shapes, same order; the deferred parameter-gradient reduction is
    documented to give the same bits)."""
    from allset_amd.han_sampling import GraphedSampledStep, load_subtensors
    B = 8
    loss_fn = torch.nn.CrossEntropyLoss()
    batches = [torch.from_numpy(np.random.default_rng(20 + i).permutation(37)[:B]).to(DEV) for i in range(5)]
    model, sampler, feats, labels, opt, n_v = _training_setup(0.0)
    model.train()
    eager = []
    for ids in batches:
        _, blocks = sampler.sample_blocks_fixed(ids)
        loss = loss_fn(model(blocks, load_subtensors(blocks, feats)), labels[ids])
        opt.zero_grad()
        loss.backward()
        opt.step()
        eager.append(loss.detach().clone())
    model2, sampler2, feats2, labels2, opt2, _ = _training_setup(0.0)
    step = GraphedSampledStep(model2, sampler2, feats2, labels2, loss_fn, opt2, B)
    assert sampler2.counter == 0
    replayed = [step(ids).detach().clone() for ids in batches]
    sampler2.check()
    assert sampler2.counter == sampler.counter == 5
    print("losses eager   ", [float(v) for v in eager])
    print("losses replayed", [float(v) for v in replayed])
    for i, (a, b) in enumerate(zip(eager, replayed)):
        assert torch.equal(a, b), f"loss of step {i}: {float(a)!r} eager, {float(b)!r} replayed"
    for (k_, p), (_, q) in zip(model.named_parameters(), model2.named_parameters()):
        assert torch.equal(p, q), f"{k_}: max |diff| {float((p - q).abs().max()):.3e}"
    assert float(eager[-1]) != float(eager[0])


def test_graphed_step_with_dropout_advances_walks_and_masks():
    from allset_amd.han_sampling import GraphedSampledStep
    model, sampler, feats, labels, opt, n_v = _training_setup(0.6)
    for grp in opt.param_groups:
        grp["lr"] = 0.0                                                               # only the walks and the masks can move the loss
    step = GraphedSampledStep(model, sampler, feats, labels, torch.nn.CrossEntropyLoss(), opt, 8)
    ids = torch.arange(8, device=DEV)
    a = float(step(ids).detach())
    b = float(step(ids).detach())
    assert a != b and sampler.counter == 2
    with pytest.raises(ValueError, match="captured at batch size 8"):
        step(ids[:5])


# ---- 6. the driver --------------------------------------------------------------------------------------------------------------
DRIVER = ["--dataset", "synthetic", "--runs", "1", "--num_epochs", "3", "--batch_size", "64", "--lr", "0.005"]


def _drive(*extra):
    from allset_amd import han_sampling as hs
    return hs.main(hs.setup(hs.build_parser().parse_args(DRIVER + list(extra)).__dict__))


def test_driver_graph_step_equals_fixed_blocks_and_the_default_is_repeatable():
    a = _drive("--graph_step", "--dropout", "0")
    b = _drive("--fixed_blocks", "--dropout", "0")
    print("train loss, --graph_step  ", a["train_loss"][0])
    print("train loss, --fixed_blocks", b["train_loss"][0])
    assert a["train_loss"] == b["train_loss"] and len(a["train_loss"][0]) == 3
    assert a["acc"] == b["acc"]
    c = _drive()                                                                      # neither flag: the driver as it was, repeatable
    d = _drive()
    assert c["train_loss"] == d["train_loss"] and c["acc"] == d["acc"] and c["macro_f1"] == d["macro_f1"]


def test_driver_graph_step_with_dropout_lowers_the_training_loss():
    a = _drive("--graph_step")
    losses = a["train_loss"][0]
    print(f"mean train loss per epoch: {['%.4f' % v for v in losses]}; test acc {a['acc'][0]:.2f}")
    assert len(losses) == 3 and losses[-1] < losses[0]
