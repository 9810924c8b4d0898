"""GPU: the degree-scaled propagate kernel (csrc/hconv.hip) and the HGNN / HCHA / HNHN baselines (allset_amd/baselines.py) against the
float64 restatement of tests/baselines_oracle.py -- kernel level, model level (eval and training mode, with the product's dropout
masks), hipGraph-captured training steps, an Adam trajectory and the train.py driver."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baselines_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)
DEV = torch.device("cuda:0")


def _hypergraph(n_v, n_e, seed, long_row=0, empty=True, isolated=0, dup=True):
    """[2, nnz] (vertex, hyperedge) pairs: random sizes 1..8, an empty interior hyperedge, a singleton, a duplicated incidence,
    optionally one hyperedge of ``long_row`` members and ``isolated`` trailing vertices without incidences."""
    rng = np.random.default_rng(seed)
    nv_used = n_v - isolated
    pairs = []
    for e in range(n_e):
        if empty and e == n_e // 2:
            continue                                               # interior empty hyperedge
        k = 1 if e == 1 else int(rng.integers(1, 9))
        pairs += [(int(v), e) for v in rng.choice(nv_used, size=min(k, nv_used), replace=False)]
    if long_row:
        pairs += [(int(v), 0) for v in rng.choice(nv_used, size=min(long_row, nv_used), replace=False)]
    if dup:
        pairs.append(pairs[3])                                     # a duplicated incidence
    ei = torch.tensor(pairs, dtype=torch.int64).t().contiguous()
    return ei


def _seeds(monkeypatch):
    from allset_amd import dense
    seeds = []
    real = dense._draw_seed

    def rec():
        s = real()
        seeds.append(s)
        return s
    monkeypatch.setattr(dense, "_draw_seed", rec)
    return seeds


def _mask(shape, p, seed):
    from allset_amd import dense
    return dense.dropout_scale(shape, p, seed, DEV).cpu().double()


# ---- kernel level --------------------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    # width, has_r, has_s, has_bias, act, p, direction
    (1, False, False, False, None, 0.0, "v2e"),
    (3, True, True, True, "elu", 0.5, "e2v"),
    (4, True, False, True, "relu", 0.0, "v2e"),
    (64, False, True, True, "elu", 0.5, "e2v"),
    (64, True, True, False, "relu", 0.5, "v2e"),
    (64, False, True, True, "elu", 0.3, "e2v"),                        # p * 256 not an integer: the 16-bit mask
    (128, True, True, True, "elu", 0.0, "v2e"),
    (128, False, True, True, "relu", 0.5, "e2v"),
    (256, True, True, True, None, 0.5, "e2v"),
    (257, True, False, True, "elu", 0.5, "v2e"),
    (257, False, True, False, "relu", 0.0, "e2v"),
]


@pytest.mark.parametrize("d,has_r,has_s,has_bias,act,p,direction", KERNEL_CASES)
def test_scaled_propagate_vs_oracle(monkeypatch, d, has_r, has_s, has_bias, act, p, direction):
    from allset_amd import Incidence, scaled_propagate
    n_v, n_e = (4200 if d in (64, 257) else 700), 300
    ei = _hypergraph(n_v, n_e, seed=d, long_row=4096 if d in (64, 257) else 0, isolated=5)
    n_e_ids = int(ei[1].max()) + 1
    inc = Incidence.from_edge_index(ei.to(DEV), n_src=n_v)
    n_s, n_t = (n_v, n_e_ids) if direction == "v2e" else (n_e_ids, n_v)
    g = torch.Generator().manual_seed(d)
    x = torch.randn(n_s, d, generator=g, dtype=torch.float64)
    r = torch.rand(n_s, generator=g, dtype=torch.float64) + 0.5 if has_r else None
    s = torch.rand(n_t, generator=g, dtype=torch.float64) + 0.5 if has_s else None
    b = torch.randn(d, generator=g, dtype=torch.float64) if has_bias else None
    G = torch.randn(n_t, d, generator=g, dtype=torch.float64)
    torch.manual_seed(d)                                  # (the dropout seed: reproducible whatever ran before)
    seeds = _seeds(monkeypatch)

    xd = x.float().to(DEV).requires_grad_(True)
    bd = b.float().to(DEV).requires_grad_(True) if b is not None else None
    f32 = lambda t: t.float().to(DEV) if t is not None else None
    y = scaled_propagate(xd, inc, direction, r=f32(r), s=f32(s), bias=bd, act=act, p=p)
    (y * G.float().to(DEV)).sum().backward()

    mask = _mask((n_t, d), p, seeds[0]) if p > 0 else None
    xo = x.clone().requires_grad_(True)
    bo = b.clone().requires_grad_(True) if b is not None else None
    gi, oi = (ei[0], ei[1]) if direction == "v2e" else (ei[1], ei[0])
    yo = orc.propagate(xo, gi, oi, n_t, r=r, s=s, bias=bo, act=act, mask=mask)
    (yo * G).sum().backward()
    torch.testing.assert_close(y.detach().cpu().double(), yo.detach(), **TOL)
    # gx of a member of the 4096-long row goes through elu'(z) of a z summed from 4096 fp32 terms (its absolute rounding error
    # ~1e-4 there): absolute tolerance relative to the gradient's scale
    torch.testing.assert_close(xd.grad.cpu().double(), xo.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(xo.grad.abs().max())))
    if b is not None:
        torch.testing.assert_close(bd.grad.cpu().double(), bo.grad, rtol=1e-4, atol=1e-3)


@pytest.mark.parametrize("has_r,act,p", [(True, "elu", 0.0), (False, "relu", 0.5), (True, None, 0.5)])
def test_scaled_propagate_short_row_variant(monkeypatch, has_r, act, p):
    """A large, low-degree incidence (mean degree < 6, > 16384 rows on both sides) takes the short-row kernel in the forward AND in
    the backward over the transposed CSR; same results, with and without r, with dropout in the short-row epilogue."""
    from allset_amd import Incidence, scaled_propagate
    rng = np.random.default_rng(3)
    n_v, n_e = 60000, 30000
    v = rng.integers(0, n_v, size=90000)
    e = rng.integers(0, n_e, size=90000)
    key = np.unique(v * n_e + e)
    ei = torch.from_numpy(np.stack([key // n_e, key % n_e]).astype(np.int64))
    n_e = int(ei[1].max()) + 1
    inc = Incidence.from_edge_index(ei.to(DEV), n_src=n_v)
    assert inc.by_dst.variant("segreduce", n_e) == 2 and inc.by_src.variant("segreduce", n_v) == 2
    g = torch.Generator().manual_seed(0)
    x = torch.randn(n_v, 64, generator=g, dtype=torch.float64)
    r = torch.rand(n_v, generator=g, dtype=torch.float64) if has_r else None
    s = torch.rand(n_e, generator=g, dtype=torch.float64)
    b = torch.randn(64, generator=g, dtype=torch.float64)
    G = torch.randn(n_e, 64, generator=g, dtype=torch.float64)
    torch.manual_seed(1)
    seeds = _seeds(monkeypatch)
    xd = x.float().to(DEV).requires_grad_(True)
    bd = b.float().to(DEV).requires_grad_(True)
    y = scaled_propagate(xd, inc, "v2e", r=r.float().to(DEV) if has_r else None, s=s.float().to(DEV), bias=bd, act=act, p=p)
    (y * G.float().to(DEV)).sum().backward()
    mask = _mask((n_e, 64), p, seeds[0]) if p > 0 else None
    xo = x.clone().requires_grad_(True)
    bo = b.clone().requires_grad_(True)
    yo = orc.propagate(xo, ei[0], ei[1], n_e, r=r, s=s, bias=bo, act=act, mask=mask)
    (yo * G).sum().backward()
    torch.testing.assert_close(y.detach().cpu().double(), yo.detach(), **TOL)
    torch.testing.assert_close(xd.grad.cpu().double(), xo.grad, **TOL)
    torch.testing.assert_close(bd.grad.cpu().double(), bo.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(bo.grad.abs().max())))


def test_empty_incidence_and_zero_rows():
    from allset_amd import ops
    from allset_amd.ops import CSR
    rowptr = torch.zeros(6, dtype=torch.int32, device=DEV)
    col = torch.zeros(0, dtype=torch.int32, device=DEV)
    csr = CSR(rowptr, col, col, 5, 3)
    x = torch.randn(3, 8, device=DEV)
    b = torch.randn(8, device=DEV)
    y = ops.hconv_propagate(csr, x, 5, bias=b, act="relu")
    torch.testing.assert_close(y, torch.relu(b).expand(5, 8))


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = dict(All_num_layers=2, dropout=0.5, MLP_hidden=32, num_features=24, num_classes=5, HCHA_symdegnorm=False,
             HNHN_alpha=-1.5, HNHN_beta=-0.5, HNHN_nonlinear_inbetween=True)
    a.update(kw)
    return SimpleNamespace(**a)


MODEL_CASES = [
    ("HCHA", dict(All_num_layers=2), True),
    ("HCHA", dict(All_num_layers=3), True),
    ("HCHA", dict(All_num_layers=1), False),
    ("HGNN", dict(All_num_layers=2, HCHA_symdegnorm=True), True),
    ("HGNN", dict(All_num_layers=2, HCHA_symdegnorm=True), False),
    ("HNHN", dict(All_num_layers=1), True),
    ("HNHN", dict(All_num_layers=2), True),
    ("HNHN", dict(All_num_layers=2, HNHN_nonlinear_inbetween=False), True),
    ("HNHN", dict(All_num_layers=2), False),
]


def _model_data(method, kw, self_loops, seed=0):
    from allset_amd.baselines import HCHA, HNHN
    from allset_amd.preprocessing import generate_norm_HCHA, generate_norm_HNHN
    args = _args(**kw)
    n_v, n_e = 400, 160
    # (HNHN: an empty hyperedge has |e|^alpha = inf, and the reference's NaN gradients follow -- kept to the self-loop-free cases)
    ei = _hypergraph(n_v, n_e, seed=seed, isolated=0 if self_loops else 3, empty=method != "HNHN" or not self_loops, dup=False)
    if self_loops:                                      # a singleton hyperedge for every vertex (Add_Self_Loops' effect)
        ei = torch.cat([ei, torch.stack([torch.arange(n_v), int(ei[1].max()) + 1 + torch.arange(n_v)])], dim=1)
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_v, args.num_features, generator=g, dtype=torch.float64)
    torch.manual_seed(seed)
    model = (HNHN if method == "HNHN" else HCHA)(args)
    for prm in model.parameters():                      # non-zero biases (the reference initialises HCHA's to zeros)
        with torch.no_grad():
            prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    data = SimpleNamespace(x=x.float().to(DEV), edge_index=ei.to(DEV), n_x=[n_v])
    norms = None
    if method == "HNHN":
        generate_norm_HNHN(None, data, args)
        norms = {k: torch.from_numpy(v) for k, v in orc.hnhn_norms_dense(ei, n_v, args.HNHN_alpha, args.HNHN_beta).items()}
    else:
        generate_norm_HCHA(data, args.HCHA_symdegnorm)
    return args, model.to(DEV), data, x, ei, norms


def _oracle_forward(method, args, sd, x, ei, norms, masks):
    if method == "HNHN":
        n = 1 if args.All_num_layers == 1 else args.All_num_layers
        return orc.hnhn_forward(sd, x, ei, norms, n, args.HNHN_nonlinear_inbetween, masks)
    n = max(args.All_num_layers, 2)
    return orc.hcha_forward(sd, x, ei, n, args.HCHA_symdegnorm, masks)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("method,kw,self_loops", MODEL_CASES)
def test_model_vs_oracle(monkeypatch, method, kw, self_loops, training):
    args, model, data, x, ei, norms = _model_data(method, kw, self_loops)
    model.train(training)
    seeds = _seeds(monkeypatch)
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()

    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    masks = None
    if training:
        width = args.MLP_hidden
        assert len(seeds) == len(model.convs) - 1
        masks = [_mask((x.shape[0], width), args.dropout, s) for s in seeds]
    xo = x.clone().requires_grad_(True)
    lo = _oracle_forward(method, args, sd, xo, ei, norms, masks)
    (lo * G).sum().backward()
    torch.testing.assert_close(logits.detach().cpu().double(), lo.detach(), **TOL)
    nan_ok = method == "HNHN" and not self_loops        # deg^beta = inf at isolated vertices: NaN gradients, as in the reference
    torch.testing.assert_close(data.x.grad.cpu().double(), xo.grad, equal_nan=nan_ok, **TOL)
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), sd[k].grad, equal_nan=nan_ok, rtol=1e-4, atol=1e-3,
                                   msg=lambda m, k=k: f"{k}: {m}")
    if nan_ok:
        assert torch.isnan(sd["convs.0.weight_v2e.weight"].grad).all()


# ---- graphs and training -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method,kw", [("HCHA", {}), ("HGNN", dict(HCHA_symdegnorm=True)), ("HNHN", {})])
def test_graphed_train_step_equals_eager(method, kw):
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    args, model, data, x, ei, norms = _model_data(method, kw, True)
    y = torch.randint(0, args.num_classes, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    import copy
    eager = copy.deepcopy(model)
    opt_e = FusedAdam(eager.parameters(), lr=0.01)
    eager.eval()                                          # dropout off: the graphed step below runs train_mode=False
    for _ in range(3):
        opt_e.zero_grad()
        with dense.deferred_param_grads():
            loss_fn(eager(data)).backward()
        opt_e.step()
    opt_g = FusedAdam(model.parameters(), lr=0.01)
    step = GraphedTrainStep(model, data, loss_fn, opt_g, train_mode=False)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("method,kw", [("HCHA", {}), ("HNHN", dict(All_num_layers=2))])
def test_adam_trajectory_follows_oracle(method, kw):
    from allset_amd.optim import FusedAdam
    args, model, data, x, ei, norms = _model_data(method, kw, True)
    model.eval()
    y = torch.randint(0, args.num_classes, (x.shape[0],), generator=torch.Generator().manual_seed(2))
    sd = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = FusedAdam(model.parameters(), lr=0.01)
    opt_o = torch.optim.Adam(list(sd.values()), lr=0.01)
    yd = y.to(DEV)
    for _ in range(12):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(data), yd).backward()
        opt.step()
        opt_o.zero_grad()
        torch.nn.functional.cross_entropy(_oracle_forward(method, args, sd, x, ei, norms, None), y).backward()
        opt_o.step()
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.detach().cpu().double(), sd[k].detach(), rtol=1e-3, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("method", [["HCHA"], ["HGNN", "--HCHA_symdegnorm"], ["HNHN"]])
def test_train_driver_end_to_end(tmp_path, method):
    cmd = [sys.executable, "-m", "allset_amd.train", "--dname", "synthetic", "--method", *method, "--epochs", "5", "--runs", "1",
           "--hip_graph", "1", "--res_root", str(tmp_path)]                 # (1: a failed capture raises instead of running eager)
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout


@pytest.mark.parametrize("method,kw", [("HCHA", {}), ("HGNN", dict(HCHA_symdegnorm=True, All_num_layers=3)), ("HNHN", {})])
def test_graphed_training_mode_step_equals_eager(monkeypatch, method, kw):
    """Dropout live (train_mode=True): one replay of the captured step equals one eager step that draws its masks from the same
    device seed counter value and the same per-site salts -- the masks of the replay come from the counter, as the capture recorded."""
    import copy
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    args, model, data, x, ei, norms = _model_data(method, kw, True)
    y = torch.randint(0, args.num_classes, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    salts = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: salts.append(real()) or salts[-1])
    step = GraphedTrainStep(model, data, loss_fn, FusedAdam(model.parameters(), lr=0.01), warmup=3)
    n_sites = len(salts) // 4                                 # three warm-up steps and the captured one
    assert n_sites == len(model.convs) - 1 and n_sites > 0
    captured = salts[-n_sites:]
    counter = step.counter.clone()                            # the value the replay's kernels read
    loss_g = step().clone()
    torch.cuda.synchronize()
    assert not torch.equal(step.counter, counter)             # the replay advanced it: the next replay draws fresh masks

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


def _fixture_cases():
    import baselines_cases as bc
    return [n for n in sorted(bc.CASES) if not bc.spec(n)["train"]]


@pytest.mark.parametrize("name", _fixture_cases())
def test_model_equals_recorded_reference(name):
    """The product (HIP kernels, fp32) against the reference's recorded eval-mode results (tests/golden/baselines_*.npz): logits,
    d/dx and every parameter gradient, the NaN gradients of HNHN at isolated vertices included.  (Training mode: the product's own
    masks against the float64 restatement, test_model_vs_oracle; the restatement against the recorded reference with explicit masks,
    tests/test_baselines_reference.py.)"""
    import baselines_cases as bc
    from allset_amd.baselines import HCHA, HNHN
    from allset_amd.preprocessing import generate_norm_HCHA, generate_norm_HNHN
    c = bc.spec(name)
    fx = bc.load([f for f, ns in bc.FILES.items() if name in ns][0])
    args = bc.args_of(c)
    x, _, n_v, _ = bc.raw_data(c)
    torch.manual_seed(c["seed"])
    model = (HNHN if c["method"] == "HNHN" else HCHA)(args)
    model.load_state_dict({k: v.float() for k, v in bc.perturb(model.state_dict(), c).items()})
    model = model.to(DEV).eval()
    data = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV).requires_grad_(True),
                           edge_index=torch.from_numpy(fx[f"{name}/edge_index"]).to(DEV), n_x=[n_v])
    if c["method"] == "HNHN":
        generate_norm_HNHN(None, data, args)
    else:
        generate_norm_HCHA(data, args.HCHA_symdegnorm)
    logits = model(data)
    G = torch.from_numpy(bc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()
    nan = c["method"] == "HNHN" and c["isolated"] > 0
    scale = lambda key: max(1.0, float(np.nanmax(np.abs(bc.result(fx, name, key)[1] if bc.result(fx, name, key)[0] == "whole"
                                                         else bc.result(fx, name, key)[1][1]))))
    bc.assert_result(logits, fx, name, "logits", rtol=1e-4, atol=1e-4 * scale("logits"))
    bc.assert_result(data.x.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"), equal_nan=nan)
    for k, p in model.named_parameters():
        bc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"), equal_nan=nan)
