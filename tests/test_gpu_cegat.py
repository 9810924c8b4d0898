"""GPU: the clique-expansion baseline CEGAT -- the GAT attention hop (csrc/gat.hip, functional.gat_propagate) against the float64
restatement of tests/cegat_oracle.py over head counts, widths, both output forms, empty and long rows, relu and dropout; its
softmax properties, run-to-run bit-identity of the gradients and the C entries' argument validation; the model in eval mode against
the REFERENCE's recorded results (tests/golden/baselines_cegat*.npz, tools/gen_cegat_fixtures.py) and in training mode ('bn'
included, with the product's hash masks) against the restatement; graphed training steps, an Adam trajectory, the train.py driver.

The leaky-relu kink: fp32 and float64 may disagree on the side of a pre-activation ``al[s] + ar[t]`` only where it is within fp32
rounding of 0.  Every comparison below asserts, from the float64 restatement alone, that the nearest pre-activation is more than
1e-5 away (an order above the rounding of these O(1) sums); the seeds are fixed so that it is."""
import copy
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cegat_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)
KINK_MARGIN = 1e-5
DEV = torch.device("cuda:0")


def _close(got, want, what):
    want = want.detach()
    print(f"{what}: max |diff| {float((got.detach().cpu().double() - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got.detach().cpu().double(), want, rtol=1e-4, atol=1e-4 * max(1.0, float(want.abs().max())),
                               msg=lambda m: f"{what}: {m}")


# ---- kernel level --------------------------------------------------------------------------------------------------------------
N_HOP = 2500
# (heads, channels, concat, act, p, long rows, seed): the seed is the first of 0, 1, 2, ... whose inputs keep every pre-activation
# 2e-5 away from 0 (found with hop_inputs and the restatement alone, on the CPU)
HOP_CASES = [(1, 1, True, None, 0.0, (), 0), (1, 7, True, "relu", 0.5, (70,), 0), (2, 3, True, "relu", 0.0, (1500,), 0),
             (4, 16, True, "relu", 0.5, (70, 1500), 1), (4, 32, True, None, 0.0, (1100,), 3), (8, 64, True, "relu", 0.5, (65, 2000), 1),
             (1, 128, True, "relu", 0.5, (), 0), (8, 16, True, None, 0.0, (70,), 3), (1, 5, False, None, 0.0, (70,), 1),
             (2, 7, False, "relu", 0.5, (1500,), 1), (4, 6, False, "relu", 0.0, (), 0), (4, 16, True, "relu", 0.3, (70, 1500), 1)]


def hop_inputs(H, C, concat, long_rows, seed, n=N_HOP):
    """Random directed edges over ``n`` ids with empty target rows and rows of the given lengths; fp32-representable float64 inputs."""
    rng = np.random.default_rng(1000 * seed + 17 * H + C)
    src = rng.integers(0, n, size=6 * n)
    dst = rng.integers(0, n, size=6 * n)
    keep = (dst % 13) != 5                                  # empty target rows
    src, dst = src[keep], dst[keep]
    for i, L in enumerate(long_rows):
        src = np.concatenate([src, rng.integers(0, n, size=L)])
        dst = np.concatenate([dst, np.full(L, i)])
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    g = torch.Generator().manual_seed(seed)
    width = H * C if concat else C
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    return ei, f(n, H * C), f(n, H), f(n, H), f(width), f(n, width)


def hop_oracle(case, mask):
    H, C, concat, act, p, long_rows, seed = case
    ei, x, al, ar, b, G = hop_inputs(H, C, concat, long_rows, seed)
    leaves = [t.clone().requires_grad_(True) for t in (x, al, ar, b)]
    rep = {}
    yo = orc.gat_hop(leaves[0], leaves[1], leaves[2], ei, N_HOP, H, 0.2, concat, leaves[3], act, mask, rep)
    (yo * G).sum().backward()
    return yo, leaves, rep


@pytest.mark.parametrize("case", HOP_CASES, ids=lambda c: f"H{c[0]}C{c[1]}{'cat' if c[2] else 'mean'}-{c[3]}-p{c[4]}")
def test_gat_propagate_vs_float64(monkeypatch, case):
    from allset_amd import Incidence, dense
    from allset_amd.functional import gat_propagate
    H, C, concat, act, p, long_rows, seed = case
    n = N_HOP
    ei, x, al, ar, b, G = hop_inputs(H, C, concat, long_rows, seed)
    inc = Incidence.from_edge_index(ei.to(DEV), n_src=n, n_dst=n)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    dv = [t.float().to(DEV).requires_grad_(True) for t in (x, al, ar, b)]
    y = gat_propagate(dv[0], dv[1], dv[2], inc, H, 0.2, concat, bias=dv[3], act=act, p=p)
    (y * G.float().to(DEV)).sum().backward()
    mask = dense.dropout_scale(tuple(y.shape), p, seeds[0], DEV).cpu().double() if p > 0 else None
    yo, leaves, rep = hop_oracle(case, mask)
    print(f"min |al[s] + ar[t]| = {rep['min_abs_logit']:.3e}")
    assert rep["min_abs_logit"] > KINK_MARGIN
    deg = torch.bincount(ei[1], minlength=n)
    assert bool((deg == 0).any()) and (not long_rows or int(deg.max()) >= max(long_rows))
    _close(y, yo, "y")
    for got, want, what in zip(dv, leaves, ("gx", "gal", "gar", "gbias")):
        _close(got.grad, want.grad, what)
    if act is None and p == 0:
        torch.testing.assert_close(y.detach()[(deg == 0).to(DEV)], dv[3].detach().expand(int((deg == 0).sum()), y.shape[1]))


def test_hop_cases_cover_the_kernel_paths():
    assert {c[0] for c in HOP_CASES} >= {1, 2, 4, 8}
    assert any(c[5] and max(c[5]) > 1024 for c in HOP_CASES) and any(c[5] and 64 < min(c[5]) <= 1024 for c in HOP_CASES)
    assert any(not c[2] for c in HOP_CASES) and any(c[1] % 4 for c in HOP_CASES) and any(c[0] * c[1] == 512 for c in HOP_CASES)


def _small_hop(H=4, C=8, n=400, seed=3):
    from allset_amd import Incidence
    rng = np.random.default_rng(seed)
    ei = torch.from_numpy(np.stack([rng.integers(0, n, 5 * n), rng.integers(0, n - 10, 5 * n)]).astype(np.int64))
    g = torch.Generator().manual_seed(seed)
    x, al, ar = (torch.randn(n, k, generator=g).to(DEV) for k in (H * C, H, H))
    return Incidence.from_edge_index(ei.to(DEV), n_src=n, n_dst=n), ei, x, al, ar


def test_softmax_rows_sum_to_one_and_ignore_a_per_target_shift():
    from allset_amd.functional import gat_propagate
    H, C = 4, 8
    inc, ei, x, al, ar = _small_hop(H, C)
    ones = torch.ones_like(x)
    y = gat_propagate(ones, al, ar, inc, H)                                   # sum_j p_j * 1
    nonempty = (torch.bincount(ei[1], minlength=x.shape[0]) > 0).to(DEV)
    assert bool((~nonempty).any())
    torch.testing.assert_close(y[nonempty], ones[nonempty], rtol=0, atol=1e-6)
    assert float(y[~nonempty].abs().max()) == 0.0
    # all logits positive: leaky_relu is the identity there, so a constant added per target (and head) cancels in the softmax
    alp, arp = al.abs() + 0.5, ar.abs() + 0.5
    shift = torch.rand(x.shape[0], H, device=DEV) * 3
    torch.testing.assert_close(gat_propagate(x, alp, arp + shift, inc, H), gat_propagate(x, alp, arp, inc, H), rtol=1e-5, atol=1e-5)


def test_large_logits_do_not_overflow():
    from allset_amd.functional import gat_propagate
    H, C = 2, 4
    inc, ei, x, al, ar = _small_hop(H, C, seed=5)
    al = al.clone()
    al[int(ei[0, 0])] = 80.0
    al[int(ei[0, 1])] = -80.0
    xd, ald, ard = x.requires_grad_(True), al.requires_grad_(True), ar.requires_grad_(True)
    y = gat_propagate(xd, ald, ard, inc, H)
    y.sum().backward()
    for t in (y, xd.grad, ald.grad, ard.grad):
        assert bool(torch.isfinite(t).all())
    xo, alo, aro = (t.detach().cpu().double() for t in (x, al, ar))
    _close(y, orc.gat_hop(xo, alo, aro, ei, x.shape[0], H), "y")
    t0 = int(ei[1, 0])                                                        # the target of the +80 source: that edge takes all the mass
    torch.testing.assert_close(y[t0], x[int(ei[0, 0])].detach(), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("concat", [True, False])
def test_backward_is_bit_identical_from_run_to_run(concat):
    from allset_amd import Incidence
    from allset_amd.functional import gat_propagate
    H, C = 4, 32
    ei, x, al, ar, b, G = hop_inputs(H, C, concat, (70, 1500), 0)
    inc = Incidence.from_edge_index(ei.to(DEV), n_src=N_HOP, n_dst=N_HOP)
    runs = []
    for _ in range(2):
        dv = [t.float().to(DEV).requires_grad_(True) for t in (x, al, ar, b)]
        y = gat_propagate(dv[0], dv[1], dv[2], inc, H, 0.2, concat, bias=dv[3], act="relu")
        (y * G.float().to(DEV)).sum().backward()
        runs.append([y.detach()] + [t.grad for t in dv])
    for a, b_ in zip(*runs):
        assert torch.equal(a, b_)


def test_c_entries_validate_their_arguments():
    from allset_amd import _lib
    lib = _lib.load()
    assert lib.allset_gat_supported() == 1
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    P, I = t.data_ptr(), i.data_ptr()

    def fwd(variant=1, nnz=0, rowptr=I, y=P, m=P, l=P, ar=P, ldx=8, ldy=8, act=0, p=0.0, H=2, C=4, n_t=2, aggpos=0, ppos=0):
        return lib.allset_gat_fwd(variant, nnz, 0, rowptr, I, P, ar, P, ldx, 0.2, 0, act, p, 0, 0, 1, y, ldy, 0, 8, aggpos, 8, ppos, m, l,
                                  n_t, 2, H, C, 0)

    def err():
        return lib.allset_last_error()

    assert fwd() == 0 and err() == b""
    torch.cuda.synchronize()
    assert fwd(rowptr=0) == -1 and b"null" in err()
    assert fwd(n_t=-1) == -1 and b"negative" in err()
    assert fwd(H=0) == -1 and b"heads" in err()
    assert fwd(H=8, C=128) == -3 and b"maximum" in err()
    assert fwd(H=128, C=1) == -3
    assert fwd(ldx=4) == -1 and b"leading dimension" in err()
    assert fwd(ldy=7) == -1 and b"leading dimension" in err()
    assert fwd(act=2) == -1 and b"act" in err()
    assert fwd(p=1.0) == -1 and b"dropout" in err()
    assert fwd(variant=3) == -1 and b"variant" in err()
    assert fwd(variant=2) == -3 and b"short-row" in err()
    assert fwd(aggpos=P) == -1 and b"go together" in err()
    assert fwd(n_t=0, rowptr=0) == 0 and err() == b""

    def stats(y=P, g=P, ldg=8, p=0.0, stats_ptr=P, H=2, C=4, n_t=2):
        return lib.allset_gat_bwd_stats(y, 8, 0, p, 0, 8, P, 8, P, g, ldg, P, P, 0.2, stats_ptr, P, n_t, H, C, 0)

    assert stats(g=0) == -1 and b"null" in err()
    assert stats(y=0) == -1 and b"null" in err()
    assert stats(ldg=4) == -1 and b"leading dimension" in err()
    assert stats(stats_ptr=P + 4) == -1 and b"aligned" in err()
    assert stats(H=0) == -1 and stats(H=4, C=256) == -3 and stats(p=-0.5) == -1
    assert stats(n_t=0, g=0) == 0

    def src(variant=1, rowptr=I, gx=P, ldx=8, ldgx=8, H=2, C=4, n_s=2, stats_ptr=P):
        return lib.allset_gat_bwd_src(variant, 0, 0, rowptr, I, P, P, P, ldx, P, 8, stats_ptr, 0.2, gx, ldgx, P, n_s, 2, H, C, 0)

    assert src() == 0 and err() == b""
    torch.cuda.synchronize()
    assert src(rowptr=0) == -1 and b"null" in err()
    assert src(gx=0) == -1 and b"null" in err()
    assert src(ldgx=4) == -1 and b"leading dimension" in err()
    assert src(n_s=-2) == -1 and src(H=1, C=1024) == -3 and src(variant=2) == -3 and src(variant=-1) == -1
    assert src(stats_ptr=P + 4) == -1 and b"aligned" in err()
    with pytest.raises(ValueError, match="act"):
        from allset_amd.functional import gat_propagate
        gat_propagate(t.view(8, 8), t[:8].view(8, 1), t[:8].view(8, 1), None, 1, act="elu")


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _hyperedges(seed, n_v=300, n_e=120, trailing=4, interior=(11, 12)):
    """(vertex, hyperedge) incidences: sizes 1..8 (a few of one member), a pair shared by three more hyperedges, vertices
    ``interior`` and the last ``trailing`` in no hyperedge."""
    rng = np.random.default_rng(seed)
    pool = np.array([v for v in range(n_v - trailing) if v not in interior])
    pairs = set()
    for e in range(n_e):
        k = 1 if e % 17 == 3 else int(rng.integers(2, 9))
        pairs |= {(int(v), e) for v in rng.choice(pool, size=k, replace=False)}
    for e in range(n_e, n_e + 3):
        pairs |= {(int(pool[0]), e), (int(pool[1]), e)}
    return torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous(), n_v


HID, NCLS = 32, 5


def _model_data(L=2, normalization="ln", heads=1, oheads=1, seed=0, dropout=0.5):
    from allset_amd.baselines import CEGAT
    from allset_amd.preprocessing import ConstructV2V, norm_contruction
    ei, n_v = _hyperedges(seed)
    data = norm_contruction(ConstructV2V(SimpleNamespace(edge_index=ei)), TYPE='V2V')
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_v, 24, generator=g, dtype=torch.float32).double()
    torch.manual_seed(seed)
    model = CEGAT(24, HID, NCLS, L, heads, oheads, dropout, Normalization=normalization)
    for prm in model.parameters():                          # non-zero biases
        with torch.no_grad():
            prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    dd = SimpleNamespace(x=x.float().to(DEV), edge_index=data.edge_index.to(DEV), norm=data.norm.to(DEV))
    return model.to(DEV), dd, x, data.edge_index.cpu()


def _sd64(model):
    return {k: (v.detach().cpu().double() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}


def _assert_model_matches(model, data, x, ei, logits, G, masks, L, heads, oheads, bn=False, training=False):
    sd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in _sd64(model).items()}
    xo = x.clone().requires_grad_(True)
    reports = []
    lo = orc.cegat_forward(sd, xo, ei, max(L, 2), heads, oheads, masks, bn=bn, training=training, reports=reports)
    (lo * G).sum().backward()
    margins = [r["min_abs_logit"] for r in reports]
    print("min |al[s] + ar[t]| per conv:", ["%.3e" % m for m in margins])
    assert min(margins) > KINK_MARGIN
    _close(logits, lo, "logits")
    _close(data.x.grad, xo.grad, "grad_x")
    for k, prm in model.named_parameters():
        _close(prm.grad, sd[k].grad, f"grad:{k}")
    return lo


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("L,heads,oheads", [(1, 4, 2), (2, 4, 1), (2, 1, 2), (3, 1, 1)])
def test_model_vs_oracle(monkeypatch, L, heads, oheads, training):
    from allset_amd import dense
    model, data, x, ei = _model_data(L, "ln", heads, oheads)
    model.train(training)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    masks = None
    if training:
        assert len(seeds) == len(model.convs) - 1
        widths = [heads * HID] + [HID] * (len(model.convs) - 2)
        masks = [dense.dropout_scale((x.shape[0], w), 0.5, s, DEV).cpu().double() for s, w in zip(seeds, widths)]
    lo = _assert_model_matches(model, data, x, ei, logits, G, masks, L, heads, oheads, training=training)
    # isolated vertices (interior 11, 12 and the trailing four): a one-entry softmax -- the output is their own transformed row
    n = x.shape[0]
    if not training and L == 1:
        sd = _sd64(model)
        h = torch.relu(x @ sd["convs.0.lin_l.weight"].t() + sd["convs.0.bias"])
        own = (h @ sd["convs.1.lin_l.weight"].t()).view(n, oheads, NCLS).mean(1) + sd["convs.1.bias"]
        for v in (11, 12, n - 1, n - 4):
            torch.testing.assert_close(lo[v].detach(), own[v], rtol=1e-10, atol=1e-10)


def test_batchnorm_model_training_with_product_masks(monkeypatch):
    """``'bn'`` in training mode: batch statistics, then the hash dropout -- its masks fed to the restatement."""
    from allset_amd import dense
    model, data, x, ei = _model_data(3, "bn")
    model.train()
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    assert len(seeds) == 2
    masks = [dense.dropout_scale((x.shape[0], HID), 0.5, s_, DEV).cpu().double() for s_ in seeds]
    _assert_model_matches(model, data, x, ei, logits, G, masks, 3, 1, 1, bn=True, training=True)


def test_batchnorm_model_eval_equals_oracle():
    model, data, x, ei = _model_data(2, "bn", 1, 2)
    model.eval()
    with torch.no_grad():
        bn = model.normalizations[0]
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    _assert_model_matches(model, data, x, ei, logits, G, None, 2, 1, 2, bn=True, training=False)


# ---- against the recorded reference (tests/golden/baselines_cegat*.npz) --------------------------------------------------------
def _eval_cases():
    import cegat_cases as gc
    return [n for n in sorted(gc.CASES) if not gc.spec(n)["train"]]


@pytest.mark.parametrize("name", _eval_cases())
def test_model_equals_recorded_reference(name):
    """The product (HIP kernels, fp32, its own device preprocessing) against the reference's recorded eval-mode results.  (Training
    mode: the product's own masks against the restatement above; the restatement against the recorded training-mode results with
    explicit masks: tests/test_cegat_reference.py.)"""
    import cegat_cases as gc
    import test_cegat_reference as ref
    from allset_amd.baselines import CEGAT
    from allset_amd.train import HypergraphData, build_model, build_parser, preprocess
    c = gc.spec(name)
    fx = gc.load(ref.FILE_OF[name])
    x, block, n_v, n_e = gc.raw_data(c)
    args = build_parser().parse_args(["--method", "CEGAT"])
    data = preprocess(args, HypergraphData(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(block), n_x=[n_v],
                                           num_hyperedges=[n_e]))
    assert data.clique_expansion
    key = lambda e: np.lexsort((np.asarray(e)[1], np.asarray(e)[0]))
    got_ei, ref_ei = data.edge_index.numpy(), fx[f"{name}/edge_index"].astype(np.int64)
    np.testing.assert_array_equal(got_ei[:, key(got_ei)], ref_ei[:, key(ref_ei)])
    _, _, _, reports = ref.oracle_run(c, fx, name)
    margins = [r["min_abs_logit"] for r in reports]
    print("min |al[s] + ar[t]| per conv:", ["%.3e" % m for m in margins])
    assert min(margins) > KINK_MARGIN
    torch.manual_seed(c["seed"])
    model = build_model(gc.args_of(c), data)
    assert isinstance(model, CEGAT)
    model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in gc.perturbed(model.state_dict(), c).items()})
    model = model.to(DEV).eval()
    dd = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV).requires_grad_(True), edge_index=data.edge_index.to(DEV),
                         norm=data.norm.to(DEV))
    logits = model(dd)
    G = torch.from_numpy(gc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()

    def scale(k):
        kind, v = gc.result(fx, name, k)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    gc.assert_result(logits, fx, name, "logits", rtol=1e-4, atol=1e-4 * scale("logits"))
    gc.assert_result(dd.x.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"))
    for k, p in model.named_parameters():
        gc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"))


# ---- training steps --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm,heads", [("ln", 4), ("bn", 1)])
def test_graphed_training_mode_step_equals_eager(monkeypatch, norm, heads):
    """Dropout (and, with 'bn', batch statistics) live: one replay of the captured step equals one eager step that draws its masks
    from the same device seed counter value and the same per-site salts."""
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    model, data, x, _ = _model_data(2, norm, heads, 2)
    y = torch.randint(0, NCLS, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    salts = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: salts.append(real()) or salts[-1])
    step = GraphedTrainStep(model, data, loss_fn, FusedAdam(model.parameters(), lr=0.01), warmup=3)
    n_sites = len(salts) // 4
    assert n_sites == len(model.convs) - 1
    captured = salts[-n_sites:]
    counter = step.counter.clone()
    loss_g = step().clone()
    torch.cuda.synchronize()
    replay_salts = iter(captured)
    monkeypatch.setattr(dense, "_draw_seed", lambda: next(replay_salts))
    opt = FusedAdam(eager.parameters(), lr=0.01)
    eager.train()
    with dense.device_seed_counter(counter):
        opt.zero_grad()
        loss_e = loss_fn(eager(data))
        loss_e.backward()
    opt.step()
    torch.testing.assert_close(loss_g, loss_e.detach(), rtol=1e-5, atol=1e-6)
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


def test_graphed_train_step_equals_eager():
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    model, data, x, _ = _model_data(2, "ln", 4, 2)
    y = torch.randint(0, NCLS, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    opt_e = FusedAdam(eager.parameters(), lr=0.01)
    eager.eval()
    for _ in range(3):
        opt_e.zero_grad()
        with dense.deferred_param_grads():
            loss_fn(eager(data)).backward()
        opt_e.step()
    step = GraphedTrainStep(model, data, loss_fn, FusedAdam(model.parameters(), lr=0.01), train_mode=False)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


def test_adam_trajectory_follows_oracle():
    from allset_amd.optim import FusedAdam
    model, data, x, ei = _model_data(2, "ln", 4, 2)
    model.eval()
    y = torch.randint(0, NCLS, (x.shape[0],), generator=torch.Generator().manual_seed(2))
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd64(model).items() if "lin_r" not in k}
    opt = FusedAdam(model.parameters(), lr=0.01)
    opt_o = torch.optim.Adam(list(sd.values()), lr=0.01)
    yd = y.to(DEV)
    for _ in range(12):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(data), yd).backward()
        opt.step()
        opt_o.zero_grad()
        torch.nn.functional.cross_entropy(orc.cegat_forward(sd, x, ei, 2, 4, 2), y).backward()
        opt_o.step()
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.detach().cpu().double(), sd[k].detach(), rtol=1e-3, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("extra", [["--heads", "4"], ["--heads", "4", "--output_heads", "2", "--hip_graph", "0"],
                                   ["--normalization", "bn", "--All_num_layers", "3"]])
def test_train_driver_end_to_end(tmp_path, extra):
    cmd = [sys.executable, "-m", "allset_amd.train", "--dname", "synthetic", "--method", "CEGAT", "--epochs", "5", "--runs", "1",
           "--res_root", str(tmp_path)] + (extra if "--hip_graph" in extra else extra + ["--hip_graph", "1"])
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout
