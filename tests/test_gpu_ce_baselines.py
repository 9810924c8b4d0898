"""GPU: the clique-expansion baseline CEGCN -- the device clique expansion and GCN normalisation (csrc/clique.hip) against the
float64 restatement of tests/ce_oracle.py, the weighted propagate (allset_hconv_fwd_w) against float64 over widths, empty and long
rows and dropout, the model in eval and training mode ('bn' included, with the product's hash masks), graphed training steps, an
Adam trajectory and the train.py driver; and the device preprocessing and the model against the REFERENCE's recorded results
(tests/golden/baselines_ce*.npz, tools/gen_ce_fixtures.py)."""
import copy
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)
DEV = torch.device("cuda:0")


def _hyperedges(seed, n_v=300, n_e=120, trailing=4, interior=(11, 12), long_edge=0):
    """(vertex, hyperedge) incidences: sizes 1..8 (a few of one member), a pair shared by three more hyperedges, vertices
    ``interior`` and the last ``trailing`` in no hyperedge, optionally one hyperedge of ``long_edge`` members."""
    rng = np.random.default_rng(seed)
    pool = np.array([v for v in range(n_v - trailing) if v not in interior])
    pairs = set()
    for e in range(n_e):
        k = 1 if e % 17 == 3 else int(rng.integers(2, 9))
        pairs |= {(int(v), e) for v in rng.choice(pool, size=k, replace=False)}
    for e in range(n_e, n_e + 3):
        pairs |= {(int(pool[0]), e), (int(pool[1]), e)}
    if long_edge:
        pairs |= {(int(v), n_e + 3) for v in rng.choice(pool, size=long_edge, replace=False)}
    return torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous(), n_v


def _canon(ei, w):
    key = ei[0] * (int(ei.max()) + 1) + ei[1]
    order = torch.argsort(key)
    return ei[:, order], w[order]


@pytest.mark.parametrize("seed,long_edge,on_host", [(0, 0, True), (1, 0, False), (2, 200, True)])
def test_clique_expansion_and_gcn_norm_equal_oracle(seed, long_edge, on_host):
    from allset_amd.preprocessing import ConstructV2V, norm_contruction
    ei, n_v = _hyperedges(seed, long_edge=long_edge)
    ei = torch.stack([ei[0], ei[1] + n_v])                  # hyperedge ids behind the vertex ids, as ExtractV2E leaves them
    data = SimpleNamespace(edge_index=ei if on_host else ei.to(DEV))
    data = ConstructV2V(data)
    assert data.edge_index.device == data.norm.device == (torch.device("cpu") if on_host else DEV)
    pairs, mult = orc.clique_expansion(ei)
    got_ei, got_m = _canon(data.edge_index.cpu(), data.norm.cpu())
    assert torch.equal(got_ei, pairs)
    assert data.norm.dtype == torch.float32 and torch.equal(got_m.double(), mult)
    assert float(mult.max()) >= 3.0
    data = norm_contruction(data, TYPE='V2V')
    want_ei, want_w = orc.gcn_norm(pairs, mult)
    got_ei, got_w = _canon(data.edge_index.cpu(), data.norm.cpu())
    want_ei, want_w = _canon(want_ei, want_w)
    assert torch.equal(got_ei, want_ei)
    torch.testing.assert_close(got_w.double(), want_w, rtol=1e-6, atol=0)
    n = int(pairs.max()) + 1
    assert n < n_v and int(data.edge_index.max()) == n - 1  # trailing isolated vertices: no loop


def test_clique_expansion_refuses_an_int32_overflow_before_emitting():
    from allset_amd.preprocessing import ConstructV2V
    k = 65537                                               # k (k - 1) / 2 = 2^31 + 32768 pairs
    ei = torch.stack([torch.arange(k), torch.full((k,), k)]).to(DEV)
    with pytest.raises(ValueError, match="int32"):
        ConstructV2V(SimpleNamespace(edge_index=ei))


# ---- kernel level --------------------------------------------------------------------------------------------------------------
def _graph(n, seed, long_rows):
    """Random directed edges over n ids with a few empty target rows and rows of the given lengths, weights in (0.5, 1.5)."""
    rng = np.random.default_rng(seed)
    src = rng.integers(0, n, size=6 * n)
    dst = rng.integers(0, n, size=6 * n)
    keep = (dst % 13) != 5                                  # empty target rows
    src, dst = src[keep], dst[keep]
    for i, L in enumerate(long_rows):
        src = np.concatenate([src, rng.integers(0, n, size=L)])
        dst = np.concatenate([dst, np.full(L, i)])
    ei = torch.from_numpy(np.stack([src, dst]).astype(np.int64))
    w = torch.from_numpy(rng.random(ei.shape[1]) + 0.5)
    return ei, w


@pytest.mark.parametrize("d,act,p,long_rows", [(1, None, 0.0, ()), (3, "relu", 0.5, (70,)), (7, "relu", 0.0, (1500,)),
                                               (64, "relu", 0.5, (70, 1500)), (128, None, 0.0, (1100,)), (128, "relu", 0.5, ()),
                                               (512, "relu", 0.5, (65, 2000)), (64, "relu", 0.3, (70, 1500))])
def test_weighted_propagate_vs_float64(monkeypatch, d, act, p, long_rows):
    from allset_amd import Incidence, dense
    from allset_amd.functional import weighted_propagate
    n = 2500
    ei, w = _graph(n, d, long_rows)
    inc = Incidence.from_edge_index(ei.to(DEV), n_src=n, n_dst=n)
    wf = w.float().to(DEV)
    w_dst, w_src = wf[inc.perm_dst_long()].contiguous(), wf[inc.perm_src_long()].contiguous()
    g = torch.Generator().manual_seed(d)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    b = torch.randn(d, generator=g, dtype=torch.float64)
    G = torch.randn(n, d, generator=g, dtype=torch.float64)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    xd = x.float().to(DEV).requires_grad_(True)
    bd = b.float().to(DEV).requires_grad_(True)
    y = weighted_propagate(xd, inc, w_dst, w_src, bias=bd, act=act, p=p)
    (y * G.float().to(DEV)).sum().backward()
    mask = dense.dropout_scale((n, d), p, seeds[0], DEV).cpu().double() if p > 0 else None
    xo = x.clone().requires_grad_(True)
    bo = b.clone().requires_grad_(True)
    yo = orc.gcn_conv(xo, ei, w, torch.eye(d, dtype=torch.float64), bo, act=act, mask=mask)
    (yo * G).sum().backward()
    scale = max(1.0, float(yo.detach().abs().max()))
    torch.testing.assert_close(y.detach().cpu().double(), yo.detach(), rtol=1e-4, atol=1e-4 * scale)
    torch.testing.assert_close(xd.grad.cpu().double(), xo.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(xo.grad.abs().max())))
    torch.testing.assert_close(bd.grad.cpu().double(), bo.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(bo.grad.abs().max())))
    empty = torch.bincount(ei[1], minlength=n) == 0
    assert bool(empty.any())
    if act is None and p == 0:
        torch.testing.assert_close(y.detach()[empty.to(DEV)], bd.detach().expand(int(empty.sum()), d))


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _model_data(L=2, normalization="ln", seed=0, dropout=0.5):
    from allset_amd.baselines import CEGCN
    from allset_amd.preprocessing import ConstructV2V, norm_contruction
    ei, n_v = _hyperedges(seed)
    data = norm_contruction(ConstructV2V(SimpleNamespace(edge_index=ei)), TYPE='V2V')
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_v, 24, generator=g, dtype=torch.float64)
    torch.manual_seed(seed)
    model = CEGCN(24, 32, 5, L, dropout, Normalization=normalization)
    for prm in model.parameters():                          # non-zero biases
        with torch.no_grad():
            prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    pairs, mult = orc.clique_expansion(ei)
    oei, ow = orc.gcn_norm(pairs, mult)
    dd = SimpleNamespace(x=x.float().to(DEV), edge_index=data.edge_index.to(DEV), norm=data.norm.to(DEV))
    return model.to(DEV), dd, x, oei, ow


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("L", [1, 2, 3])
def test_model_vs_oracle(monkeypatch, L, training):
    from allset_amd import dense
    model, data, x, oei, ow = _model_data(L)
    model.train(training)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    masks = None
    if training:
        assert len(seeds) == len(model.convs) - 1
        masks = [dense.dropout_scale((x.shape[0], 32), 0.5, s, DEV).cpu().double() for s in seeds]
    xo = x.clone().requires_grad_(True)
    lo = orc.cegcn_forward(sd, xo, oei, ow, len(model.convs), masks)
    (lo * G).sum().backward()
    torch.testing.assert_close(logits.detach().cpu().double(), lo.detach(), **TOL)
    torch.testing.assert_close(data.x.grad.cpu().double(), xo.grad, **TOL)
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), sd[k].grad, rtol=1e-4, atol=1e-3, msg=lambda m, k=k: f"{k}: {m}")
    n = int(oei.max()) + 1
    torch.testing.assert_close(logits.detach()[n:], model.convs[-1].bias.detach().expand(x.shape[0] - n, 5))


def test_batchnorm_model_training_with_product_masks(monkeypatch):
    """``'bn'`` in training mode: batch statistics, then the hash dropout -- its masks fed to the restatement."""
    from allset_amd import dense
    model, data, x, oei, ow = _model_data(3, "bn")
    model.train()
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    assert len(seeds) == 2
    masks = [dense.dropout_scale((x.shape[0], 32), 0.5, s_, DEV).cpu().double() for s_ in seeds]
    sd = {k: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    lo = orc.cegcn_forward(sd, xo, oei, ow, 3, masks, bn=True, training=True)
    (lo * G).sum().backward()
    torch.testing.assert_close(logits.detach().cpu().double(), lo.detach(), **TOL)
    torch.testing.assert_close(data.x.grad.cpu().double(), xo.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(xo.grad.abs().max())))
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), sd[k].grad, rtol=1e-4, atol=1e-3, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("norm", ["ln", "bn"])
def test_graphed_training_mode_step_equals_eager(monkeypatch, norm):
    """Dropout (and, with 'bn', batch statistics) live: one replay of the captured step equals one eager step that draws its masks
    from the same device seed counter value and the same per-site salts."""
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    model, data, x, _, _ = _model_data(3, norm)
    y = torch.randint(0, 5, (x.shape[0],), device=DEV)
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


# ---- against the recorded reference (tests/golden/baselines_ce*.npz) ----------------------------------------------------------
def _fixture(name):
    import ce_cases as cc
    return cc.spec(name), cc.load([f for f, ns in cc.FILES.items() if name in ns][0])


def _canon_np(ei, w):
    ei, w = np.asarray(ei), np.asarray(w)
    order = np.lexsort((ei[1], ei[0]))
    return ei[:, order], w[order]


def _preprocessed(c):
    import ce_cases as cc
    from allset_amd.train import HypergraphData, build_parser, preprocess
    x, block, n_v, n_e = cc.raw_data(c)
    args = build_parser().parse_args(["--method", "CEGCN"])
    data = HypergraphData(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e])
    return preprocess(args, data), x


@pytest.mark.parametrize("name", sorted(__import__("ce_cases").CASES))
def test_device_preprocessing_equals_recorded_reference(name):
    c, fx = _fixture(name)
    data, _ = _preprocessed(c)
    assert data.edge_index.device.type == "cpu" and data.clique_expansion
    got_ei, got_w = _canon_np(data.edge_index.numpy(), data.norm.numpy())
    ref_ei, ref_w = _canon_np(fx[f"{name}/edge_index"], fx[f"{name}/norm"])
    np.testing.assert_array_equal(got_ei, ref_ei)
    np.testing.assert_allclose(got_w, ref_w, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", [n for n in sorted(__import__("ce_cases").CASES) if not __import__("ce_cases").spec(n)["train"]])
def test_model_equals_recorded_reference(name):
    """The product (HIP kernels, fp32, its own device preprocessing) against the reference's recorded eval-mode results.  (Training
    mode: the product's own masks against the restatement above; the restatement against the recorded training-mode results with
    explicit masks: tests/test_ce_reference.py.)"""
    import ce_cases as cc
    c, fx = _fixture(name)
    data, x = _preprocessed(c)
    args = cc.args_of(c)
    torch.manual_seed(c["seed"])
    from allset_amd.baselines import CEGCN
    model = CEGCN(args.num_features, args.MLP_hidden, args.num_classes, args.All_num_layers, args.dropout, args.normalization)
    model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in cc.perturb(model.state_dict(), c).items()})
    model = model.to(DEV).eval()
    dd = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV).requires_grad_(True), edge_index=data.edge_index.to(DEV),
                         norm=data.norm.to(DEV))
    logits = model(dd)
    G = torch.from_numpy(cc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()

    def scale(key):
        kind, v = cc.result(fx, name, key)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    cc.assert_result(logits, fx, name, "logits", rtol=1e-4, atol=1e-4 * scale("logits"))
    cc.assert_result(dd.x.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"))
    for k, p in model.named_parameters():
        cc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"))


def test_batchnorm_model_eval_equals_oracle():
    """``'bn'``: relu in the conv's launch, then the BatchNorm (running statistics in eval) before the next conv."""
    model, data, x, oei, ow = _model_data(2, "bn")
    model.eval()
    with torch.no_grad():
        bn = model.normalizations[0]
        bn.running_mean.uniform_(-0.2, 0.2)
        bn.running_var.uniform_(0.5, 1.5)
    logits = model(data)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    h = orc.gcn_conv(x, oei, ow, sd["convs.0.weight"], sd["convs.0.bias"], act="relu")
    h = (h - sd["normalizations.0.running_mean"]) / torch.sqrt(sd["normalizations.0.running_var"] + 1e-5)
    h = h * sd["normalizations.0.weight"] + sd["normalizations.0.bias"]
    lo = orc.gcn_conv(h, oei, ow, sd["convs.1.weight"], sd["convs.1.bias"])
    torch.testing.assert_close(logits.detach().cpu().double(), lo, **TOL)


def test_graphed_train_step_equals_eager():
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    model, data, x, _, _ = _model_data(2)
    y = torch.randint(0, 5, (x.shape[0],), device=DEV)
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
    model, data, x, oei, ow = _model_data(2)
    model.eval()
    y = torch.randint(0, 5, (x.shape[0],), generator=torch.Generator().manual_seed(2))
    sd = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.state_dict().items()}
    opt = FusedAdam(model.parameters(), lr=0.01)
    opt_o = torch.optim.Adam(list(sd.values()), lr=0.01)
    yd = y.to(DEV)
    for _ in range(12):
        opt.zero_grad()
        torch.nn.functional.cross_entropy(model(data), yd).backward()
        opt.step()
        opt_o.zero_grad()
        torch.nn.functional.cross_entropy(orc.cegcn_forward(sd, x, oei, ow, 2), y).backward()
        opt_o.step()
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.detach().cpu().double(), sd[k].detach(), rtol=1e-3, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("extra", [[], ["--normalization", "bn"]])
def test_train_driver_end_to_end(tmp_path, extra):
    cmd = [sys.executable, "-m", "allset_amd.train", "--dname", "synthetic", "--method", "CEGCN", "--epochs", "5", "--runs", "1",
           "--hip_graph", "1", "--res_root", str(tmp_path)] + extra
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout
