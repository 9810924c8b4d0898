"""GPU: the UniGCNII baseline -- the fused E->V hop (csrc/unigcn.hip, functional.unigcn_hop) against the float64 restatement of
tests/unigcnii_oracle.py over the built widths (4 .. 512), an unsupported width and a width above 512 through the unfused fallback,
empty rows, rows longer than 64 and than 1024, both kernel variants (chosen by hand and by the mean degree), ``use_norm`` on and off and
two values of ``alpha``; the row-norm scale as a constant of the backward; run-to-run bit-identity; the C entry's argument validation;
the model in eval mode against the REFERENCE's recorded results (tests/golden/baselines_unigcnii*.npz, tools/gen_unigcnii_fixtures.py)
and in training mode (the product's hash masks, both arithmetic modes) against the restatement; graphed training steps, an Adam
trajectory with the two weight-decay groups, the train.py driver.

The relu kink: fp32 and float64 may disagree on the side of a pre-activation only where it is within fp32 rounding of 0.  Every model
comparison asserts, from the float64 restatement alone, that the smallest non-zero ``|pre-activation| / (largest of its row)`` exceeds
``unigcnii_cases.RELU_MARGIN`` (tests/util.py::oracle_relu_margin's criterion and bound); the seeds are fixed."""
import copy
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unigcnii_cases as uc  # noqa: E402
import unigcnii_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _close(got, want, what):
    want = want.detach()
    print(f"{what}: max |diff| {float((got.detach().cpu().double() - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got.detach().cpu().double(), want, rtol=1e-4, atol=1e-4 * max(1.0, float(want.abs().max())),
                               msg=lambda m: f"{what}: {m}")


# ---- kernel level --------------------------------------------------------------------------------------------------------------
# (width, use_norm, alpha, long rows, variant (None: the library's choice), vertices, incidences per vertex)
HOP_CASES = [(4, True, 0.1, (), None, 2500, 6), (12, False, 0.1, (70,), None, 2500, 6), (64, True, 0.25, (70, 1500), None, 2500, 6),
             (128, True, 0.1, (1100,), None, 2500, 6), (256, False, 0.1, (65, 2000), None, 2500, 6),
             (512, True, 0.1, (70, 1500), None, 2500, 6), (512, False, 0.3, (), None, 2500, 6), (320, True, 0.1, (70,), None, 2500, 6),
             (6, True, 0.1, (70,), None, 2500, 6), (520, False, 0.1, (), None, 2500, 3),
             (12, True, 0.1, (), 2, 2500, 6), (64, True, 0.1, (70,), 2, 2500, 6), (256, False, 0.25, (), 2, 2500, 3),
             (32, True, 0.1, (70,), None, 20000, 3), (32, True, 0.1, (1500,), None, 20000, 9)]


def hop_inputs(d, long_rows, n, per_row, seed=0):
    """Random (vertex, hyperedge) incidences over ``n`` vertices and ``n`` hyperedges with empty vertex rows and rows of the given
    lengths; fp32-representable float64 inputs."""
    rng = np.random.default_rng(1000 * seed + d)
    V = rng.integers(0, n, size=per_row * n)
    E = rng.integers(0, n, size=per_row * n)
    keep = (V % 13) != 5                                    # empty vertex rows
    V, E = V[keep], E[keep]
    for i, L in enumerate(long_rows):
        V = np.concatenate([V, np.full(L, i)])
        E = np.concatenate([E, rng.integers(0, n, size=L)])
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    degV = (0.2 + torch.rand(n, generator=g, dtype=torch.float32)).double()
    return torch.from_numpy(V.astype(np.int64)), torch.from_numpy(E.astype(np.int64)), f(n, d), f(n, d), degV, f(n, d)


def _hop_ids(c):
    return f"d{c[0]}-{'norm' if c[1] else 'plain'}-a{c[2]}-v{c[4]}-n{c[5]}x{c[6]}"


@pytest.mark.parametrize("case", HOP_CASES, ids=_hop_ids)
def test_unigcn_hop_vs_float64(case):
    from allset_amd import Incidence, ops
    from allset_amd.functional import unigcn_hop
    d, use_norm, alpha, long_rows, variant, n, per_row = case
    V, E, xe, x0, degV, G = hop_inputs(d, long_rows, n, per_row)
    inc = Incidence.from_edge_index(torch.stack([V, E]).to(DEV), n_src=n, n_dst=n)
    deg = torch.bincount(V, minlength=n)
    assert bool((deg == 0).any()) and (not long_rows or int(deg.max()) >= max(long_rows))
    built = d % 4 == 0 and d <= 512
    assert ops.unigcn_hop_supported(xe.float().to(DEV), x0.float().to(DEV)) == built
    if variant is None and built and d <= 256:               # the library's choice follows the mean degree above 16384 rows
        assert inc.by_src.variant("segreduce", n) == (2 if (n > 16384 and V.numel() < 6 * n) else 1)
    dv = [t.float().to(DEV).requires_grad_(True) for t in (xe, x0)]
    y = unigcn_hop(dv[0], dv[1], inc, degV.float().to(DEV), alpha, use_norm, variant=variant)
    (y * G.float().to(DEV)).sum().backward()
    leaves = [t.clone().requires_grad_(True) for t in (xe, x0)]
    rep = {}
    yo = orc.hop(leaves[0], leaves[1], V, E, degV, alpha, use_norm, report=rep)
    (yo * G).sum().backward()
    _close(y, yo, "Xi")
    _close(dv[0].grad, leaves[0].grad, "gxe")
    _close(dv[1].grad, leaves[1].grad, "gx0")
    empty = (deg == 0).to(DEV)
    torch.testing.assert_close(y.detach()[empty], (dv[1].detach() * alpha)[empty], rtol=1e-6, atol=1e-7)      # a = 0: Xi = alpha * x0
    if built:
        xi, t = ops.unigcn_hop_fwd(inc.by_src, dv[0].detach(), dv[1].detach(), n, degV.float().to(DEV), alpha, use_norm, variant)
        assert torch.equal(xi, y.detach())
        if use_norm:
            _close(t, rep["t"], "t")
            assert float(t[empty].abs().max()) == 0.0
        else:
            assert t is None
    if use_norm:
        # the scale is a CONSTANT of the backward: differentiating through the norm gives another gxe, further away than the tolerance
        other = xe.clone().requires_grad_(True)
        (orc.hop(other, x0, V, E, degV, alpha, True, detach=False) * G).sum().backward()
        want = leaves[0].grad
        gap = float((other.grad - want).abs().max())
        print(f"gxe through the norm differs by {gap:.3e}")
        assert gap > 100 * 1e-4 * max(1.0, float(want.abs().max()))


def test_hop_cases_cover_the_kernel_paths():
    widths = {c[0] for c in HOP_CASES}
    assert widths >= {4, 12, 64, 128, 256, 512} and any(w % 4 for w in widths) and any(w > 512 for w in widths)
    assert any(256 < w < 512 for w in widths)
    assert any(c[3] and max(c[3]) > 1024 for c in HOP_CASES) and any(c[3] and 64 < min(c[3]) <= 1024 for c in HOP_CASES)
    assert {c[1] for c in HOP_CASES} == {True, False} and len({c[2] for c in HOP_CASES}) >= 2
    assert any(c[4] == 2 for c in HOP_CASES)
    assert any(c[5] > 16384 and c[6] < 6 for c in HOP_CASES) and any(c[5] > 16384 and c[6] > 6 for c in HOP_CASES)


@pytest.mark.parametrize("d,variant", [(128, None), (512, None), (64, 2)])
def test_hop_is_bit_identical_from_run_to_run(d, variant):
    from allset_amd import Incidence
    from allset_amd.functional import unigcn_hop
    n = 2500
    V, E, xe, x0, degV, G = hop_inputs(d, (70, 1500), n, 6)
    inc = Incidence.from_edge_index(torch.stack([V, E]).to(DEV), n_src=n, n_dst=n)
    runs = []
    for _ in range(2):
        dv = [t.float().to(DEV).requires_grad_(True) for t in (xe, x0)]
        y = unigcn_hop(dv[0], dv[1], inc, degV.float().to(DEV), 0.1, True, variant=variant)
        (y * G.float().to(DEV)).sum().backward()
        runs.append([y.detach()] + [t.grad for t in dv])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_x0_gradient_accumulates_over_the_layers_in_one_buffer():
    """``initial_residual``: the hops of a forward add their ``alpha * gXi`` into one buffer; the sum equals autograd's own."""
    from allset_amd import Incidence
    from allset_amd.functional import initial_residual, unigcn_hop
    n, d = 2500, 64
    V, E, xe, x0, degV, G = hop_inputs(d, (70,), n, 6)
    inc = Incidence.from_edge_index(torch.stack([V, E]).to(DEV), n_src=n, n_dst=n)
    dg, Gd = degV.float().to(DEV), G.float().to(DEV)
    grads = []
    for tagged in (False, True):
        a, b = xe.float().to(DEV).requires_grad_(True), x0.float().to(DEV).requires_grad_(True)
        src = initial_residual(b * 1.0) if tagged else b * 1.0
        assert (getattr(src, "_allset_grad_sink", None) is not None) == tagged
        y = unigcn_hop(a, src, inc, dg, 0.1, True) + unigcn_hop(a * 2, src, inc, dg, 0.3, False) + 0.5 * src
        (y * Gd).sum().backward()
        grads.append((a.grad, b.grad))
    torch.testing.assert_close(grads[0][0], grads[1][0], rtol=0, atol=0)
    torch.testing.assert_close(grads[0][1], grads[1][1], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(grads[1][1], Gd * (0.1 + 0.3 + 0.5), rtol=1e-6, atol=1e-6)


def test_c_entry_validates_its_arguments():
    from allset_amd import _lib
    from allset_amd.functional import unigcn_hop
    lib = _lib.load()
    assert lib.allset_unigcn_supported() == 1
    t = torch.zeros(64, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    P, I = t.data_ptr(), i.data_ptr()

    def hop(variant=1, nnz=0, rowptr=I, xe=P, x0=P, xi=P, t_out=P, ldxe=8, ldx0=8, ldxi=8, use_norm=1, d=8, n_t=2, n_s=2):
        return lib.allset_unigcn_hop_fwd(variant, nnz, 0, rowptr, I, P, xe, ldxe, x0, ldx0, 0.1, use_norm, xi, ldxi, t_out, n_t, n_s, d, 0)

    def err():
        return lib.allset_last_error()

    assert hop() == 0 and err() == b""
    assert hop(variant=2) == 0 and hop(variant=0) == 0
    torch.cuda.synchronize()
    assert hop(rowptr=0) == -1 and b"null" in err()
    assert hop(xi=0) == -1 and b"null" in err()
    assert hop(x0=0) == -1 and b"null" in err()
    assert hop(t_out=0) == -1 and b"t_out" in err()
    assert hop(t_out=0, use_norm=0) == 0 and err() == b""
    assert hop(nnz=1, xe=0) == -1 and b"null" in err()
    assert hop(n_t=-1) == -1 and b"negative" in err()
    assert hop(ldxe=4) == -1 and b"leading dimension" in err()
    assert hop(ldx0=4) == -1 and hop(ldxi=4) == -1
    assert hop(variant=3) == -1 and b"variant" in err()
    assert hop(d=6) == -3 and b"not built" in err()
    assert hop(d=516, ldxe=516, ldx0=516, ldxi=516) == -3 and b"not built" in err()
    assert hop(d=320, ldxe=320, ldx0=320, ldxi=320, variant=2) == -3 and b"short-row" in err()
    assert hop(ldxe=10) == -3 and b"aligned" in err()
    assert hop(x0=P + 4) == -3 and b"aligned" in err()
    assert hop(n_t=0, rowptr=0) == 0 and err() == b""
    torch.cuda.synchronize()
    with pytest.raises(_lib.AllSetHipError):
        unigcn_hop(torch.zeros(2, 8), torch.zeros(2, 8), None, torch.ones(2), 0.1, False)          # CPU tensors


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _hyperedges(seed, n_v=300, n_e=120, trailing=4, interior=(11, 12)):
    """(vertex, hyperedge) incidences: sizes 1..8 (a few of one member), vertices ``interior`` and the last ``trailing`` in no
    hyperedge, one incidence twice; hyperedge ids start at 1000."""
    rng = np.random.default_rng(seed)
    pool = np.array([v for v in range(n_v - trailing) if v not in interior])
    rows = []
    for e in range(n_e):
        k = 1 if e % 17 == 3 else int(rng.integers(2, 9))
        rows += [(int(v), 1000 + e) for v in rng.choice(pool, size=k, replace=False)]
    rows.append(rows[0])
    return torch.tensor(rows, dtype=torch.int64).t().contiguous(), n_v


HID, NCLS, NFEAT = 16, 5, 24


def _model_data(L=2, heads=2, use_norm=False, seed=0):
    from allset_amd.baselines import UniGCNII
    from allset_amd.preprocessing import ConstructH_pairs, generate_norm_UniGNN
    v2e, n_v = _hyperedges(seed)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_v, NFEAT, generator=g, dtype=torch.float32).double()
    args = SimpleNamespace(method="UniGCNII", UniGNN_use_norm=use_norm)
    data = ConstructH_pairs(SimpleNamespace(x=x, edge_index=v2e))
    generate_norm_UniGNN(data, args)
    torch.manual_seed(seed)
    model = UniGCNII(args, NFEAT, HID, NCLS, L, heads, data.edge_index[0], data.edge_index[1])
    for prm in model.parameters():
        with torch.no_grad():
            prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    args.UniGNN_degV, args.UniGNN_degE = args.UniGNN_degV.to(DEV), args.UniGNN_degE.to(DEV)
    H = orc.dense_incidence(v2e, n_v)
    assert bool((H.sum(1) == 0).any())
    return model.to(DEV), SimpleNamespace(x=x.float().to(DEV)), x, H


def _sd64(model):
    return {k: v.detach().cpu().double() for k, v in model.state_dict().items()}


def _assert_model_matches(model, data, x, H, logits, G, masks, L, use_norm):
    sd = {k: v.requires_grad_(True) for k, v in _sd64(model).items()}
    xo = x.clone().requires_grad_(True)
    V, E = orc.pairs(H)
    degV, degE = orc.degrees(H)
    margins = []
    lo = orc.forward(sd, xo, V, E, degV, degE, L, use_norm, masks, margins)
    (lo * G).sum().backward()
    print("relu margins:", ["%.3e" % m for m in margins])
    assert min(margins) > uc.RELU_MARGIN
    _close(logits, lo, "logits")
    _close(data.x.grad, xo.grad, "grad_x")
    for k, prm in model.named_parameters():
        _close(prm.grad, sd[k].grad, f"grad:{k}")


@pytest.mark.parametrize("arith", ["auto", "bf16x6"])
@pytest.mark.parametrize("L,heads,use_norm", [(1, 1, False), (2, 2, True), (4, 2, False), (4, 1, True)])
def test_training_mode_model_with_product_masks(monkeypatch, L, heads, use_norm, arith):
    from allset_amd import dense
    model, data, x, H = _model_data(L, heads, use_norm)
    model.train()
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    data.x.requires_grad_(True)
    with dense.arithmetic(arith):
        logits = model(data)
        G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
        (logits * G.float().to(DEV)).sum().backward()
    assert len(seeds) == L + 2
    shapes = [(x.shape[0], NFEAT)] + [(x.shape[0], HID * heads)] * (L + 1)
    masks = [dense.dropout_scale(s, 0.2, sd_, DEV).cpu().double() for s, sd_ in zip(shapes, seeds)]
    assert 0.7 < float((masks[1] > 0).double().mean()) < 0.9
    _assert_model_matches(model, data, x, H, logits, G, masks, L, use_norm)


@pytest.mark.parametrize("use_norm", [False, True])
def test_eval_mode_model_vs_oracle(use_norm):
    model, data, x, H = _model_data(2, 2, use_norm)
    model.eval()
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    _assert_model_matches(model, data, x, H, logits, G, None, 2, use_norm)
    assert model.graph(data.x) is model.graph(data.x)                                # built once


# ---- against the recorded reference (tests/golden/baselines_unigcnii*.npz) -----------------------------------------------------
def _eval_cases():
    return [n for n in sorted(uc.CASES) if not uc.spec(n)["train"]]


@pytest.mark.parametrize("name", _eval_cases())
def test_model_equals_recorded_reference(name):
    """The product (HIP kernels, fp32, its own preprocessing) against the reference's recorded eval-mode results.  (Training mode:
    the product's own masks against the restatement above; the restatement against the recorded training-mode results with explicit
    masks: tests/test_unigcnii_reference.py.)"""
    import test_unigcnii_reference as ref
    from allset_amd.baselines import UniGCNII
    from allset_amd.train import HypergraphData, build_model, build_parser, preprocess
    c = uc.spec(name)
    fx = uc.load(ref.FILE_OF[name])
    x, block, n_v, n_e = uc.raw_data(c)
    args = build_parser().parse_args(["--method", "UniGCNII", "--All_num_layers", str(c["L"]), "--MLP_hidden", str(c["hidden"]),
                                      "--heads", str(c["heads"])] + ([] if c["self_loops"] else ["--add_self_loop"])
                                     + (["--UniGNN_use-norm"] if c["use_norm"] else []))
    args.num_features, args.num_classes = c["F"], c["C"]
    data = preprocess(args, HypergraphData(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(block), n_x=[n_v],
                                           num_hyperedges=[n_e]))
    np.testing.assert_array_equal(data.edge_index.numpy(), fx[f"{name}/pairs"].astype(np.int64))
    _, _, _, margins = ref.oracle_run(c, fx, name)
    print("relu margins:", ["%.3e" % m for m in margins])
    assert min(margins) > uc.RELU_MARGIN
    torch.manual_seed(c["seed"])
    model = build_model(args, data)
    assert isinstance(model, UniGCNII)
    model.load_state_dict({k: v.float() for k, v in uc.perturb(model.state_dict(), c).items()})
    model = model.to(DEV).eval()
    args.UniGNN_degV, args.UniGNN_degE = args.UniGNN_degV.to(DEV), args.UniGNN_degE.to(DEV)
    dd = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV).requires_grad_(True))
    logits = model(dd)
    G = torch.from_numpy(uc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()

    def scale(k):
        kind, v = uc.result(fx, name, k)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    uc.assert_result(logits, fx, name, "logits", rtol=1e-4, atol=1e-4 * scale("logits"))
    uc.assert_result(dd.x.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"))
    for k, p in model.named_parameters():
        uc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"))


# ---- training steps --------------------------------------------------------------------------------------------------------------
def _two_group_adam(model):
    from allset_amd.train import make_optimizer
    return make_optimizer(SimpleNamespace(method="UniGCNII"), model)


@pytest.mark.parametrize("use_norm", [False, True])
def test_graphed_training_mode_step_equals_eager(monkeypatch, use_norm):
    """Dropout live: one replay of the captured step equals one eager step that draws its masks from the same device seed counter value
    and the same per-site salts; the optimizer has the two weight-decay groups."""
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    model, data, x, _ = _model_data(2, 2, use_norm)
    y = torch.randint(0, NCLS, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    salts = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: salts.append(real()) or salts[-1])
    step = GraphedTrainStep(model, data, loss_fn, _two_group_adam(model), warmup=3)
    n_sites = len(salts) // 4
    assert n_sites == 4
    captured = salts[-n_sites:]
    counter = step.counter.clone()
    loss_g = step().clone()
    torch.cuda.synchronize()
    replay_salts = iter(captured)
    monkeypatch.setattr(dense, "_draw_seed", lambda: next(replay_salts))
    opt = _two_group_adam(eager)
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
    model, data, x, _ = _model_data(4, 2, True)
    y = torch.randint(0, NCLS, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    opt_e = _two_group_adam(eager)
    eager.eval()
    for _ in range(3):
        opt_e.zero_grad()
        with dense.deferred_param_grads():
            loss_fn(eager(data)).backward()
        opt_e.step()
    step = GraphedTrainStep(model, data, loss_fn, _two_group_adam(model), train_mode=False)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


def test_adam_trajectory_follows_oracle():
    """Twelve eval-mode steps of the two-group FusedAdam against torch.optim.Adam on the float64 restatement with the same groups."""
    model, data, x, H = _model_data(2, 2, True)
    model.eval()
    y = torch.randint(0, NCLS, (x.shape[0],), generator=torch.Generator().manual_seed(2))
    sd = {k: v.clone().requires_grad_(True) for k, v in _sd64(model).items()}
    V, E = orc.pairs(H)
    degV, degE = orc.degrees(H)
    opt = _two_group_adam(model)
    reg = [v for k, v in sd.items() if ".W." in k]
    non = [v for k, v in sd.items() if ".W." not in k]
    assert len(reg) == 2 and len(non) == 4
    opt_o = torch.optim.Adam([dict(params=reg, weight_decay=0.01), dict(params=non, weight_decay=5e-4)], lr=0.01)
    yd = y.to(DEV)
    for _ in range(12):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(data), yd).backward()
        opt.step()
        opt_o.zero_grad()
        torch.nn.functional.cross_entropy(orc.forward(sd, x, V, E, degV, degE, 2, True), y).backward()
        opt_o.step()
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.detach().cpu().double(), sd[k].detach(), rtol=1e-3, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("extra", [[], ["--UniGNN_use-norm"], ["--hip_graph", "0", "--All_num_layers", "4", "--heads", "2"]])
def test_train_driver_end_to_end(tmp_path, extra):
    cmd = [sys.executable, "-m", "allset_amd.train", "--method", "UniGCNII", "--dname", "synthetic", "--epochs", "5", "--runs", "1",
           "--res_root", str(tmp_path)] + (extra if "--hip_graph" in extra else extra + ["--hip_graph", "1"])
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout
