"""GPU: the hypergraph attention kernels (csrc/hattn.hip) behind ``functional.hattn_propagate``, ``HypergraphAttentionConv``
and the attention HCHA model against the float64 restatement of tests/hcha_attn_oracle.py and the recorded reference
(tests/golden/baselines_hcha_attn.npz) -- kernel level, layer and model level (eval and training mode, with the product's masks
rebuilt from the recorded seeds), hipGraph-captured training steps, an Adam trajectory and the train.py driver."""
import copy
import os
import subprocess
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcha_attn_cases as hc  # noqa: E402
import hcha_attn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=1e-4, atol=1e-4)
PTOL = dict(rtol=1e-4, atol=1e-3)
DEV = torch.device("cuda:0")


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


def _gtol(ref):
    """Gradients through rows that sum hundreds to thousands of fp32 terms: absolute tolerance relative to the gradient's scale."""
    return dict(rtol=1e-4, atol=1e-4 * max(1.0, float(ref.abs().max())))


# ---- kernel level --------------------------------------------------------------------------------------------------------------
_GRAPHS = {}


def _graph(large):
    """The base graph (700 vertices, 300 hyperedges of 1..8 members: an empty interior hyperedge, a singleton, a duplicated incidence,
    5 trailing isolated vertices, vertex 0 in every hyperedge) or the large one (4200 vertices, hyperedge 0 with 4096 members)."""
    if large not in _GRAPHS:
        from allset_amd import Incidence
        n_v = 4200 if large else 700
        ei = hc.hypergraph(n_v, 300, seed=17 + large, empty=True, isolated=5, dup=True, hub=not large, long_row=4096 if large else 0)
        _GRAPHS[large] = (n_v, ei, Incidence.from_edge_index(ei.to(DEV), n_src=n_v, n_dst=300))
    return _GRAPHS[large]


KERNEL_CASES = [
    # H, F, concat, act, p, p_attn, attributed ze, large graph
    (1, 1, True, None, 0.0, 0.0, False, False),
    (1, 64, False, "elu", 0.5, 0.5, True, True),
    (4, 16, True, "elu", 0.5, 0.0, True, False),
    (4, 16, True, "elu", 0.3, 0.3, True, False),                       # p * 256 not an integer: the 16-bit mask, both sites
    (3, 5, False, None, 0.0, 0.5, False, False),
    (8, 32, True, "elu", 0.0, 0.5, False, False),
    (2, 128, False, None, 0.5, 0.0, True, False),
    (8, 64, True, "elu", 0.5, 0.5, False, True),
    (3, 5, True, "elu", 0.5, 0.5, True, False),
    (4, 16, False, None, 0.0, 0.0, False, False),
]


def _kernel_inputs(H, F, concat, large):
    n_v, ei, inc = _graph(large)
    n_e = 300
    g = torch.Generator().manual_seed(100 * H + F)
    z = torch.randn(n_v, H * F, generator=g, dtype=torch.float64)
    ze = torch.randn(n_e, H * F, generator=g, dtype=torch.float64)
    att = torch.randn(1, H, 2 * F, generator=g, dtype=torch.float64) * 0.5
    bias = torch.randn(H * F if concat else F, generator=g, dtype=torch.float64)
    G = torch.randn(n_v, H * F if concat else F, generator=g, dtype=torch.float64)
    D, B = orc.scales(ei, n_v, n_e, torch.rand(n_e, generator=g, dtype=torch.float64) + 0.5)
    return n_v, n_e, ei, inc, z, ze, att, bias, G, D, B


def _logits(z, ze, att, n_e, H, F, attributed):
    av = (z.view(-1, H, F) * att[:, :, :F]).sum(-1)
    src = ze if attributed else z[:n_e]
    return av, (src.view(n_e, H, F) * att[:, :, F:]).sum(-1)


def _run_kernel(monkeypatch, H, F, concat, act, p, p_attn, attributed, large, softmax_by="vertex"):
    from allset_amd import hattn_propagate
    n_v, n_e, ei, inc, z, ze, att, bias, G, D, B = _kernel_inputs(H, F, concat, large)
    torch.manual_seed(H * F)
    seeds = _seeds(monkeypatch)
    dev = [t.float().to(DEV).requires_grad_(True) for t in (z, ze, att, bias)]
    av, ae = _logits(dev[0], dev[1], dev[2], n_e, H, F, attributed)
    y = hattn_propagate(dev[0], av, ae, inc, H, D.float().to(DEV), B.float().to(DEV), 0.2, concat, bias=dev[3], act=act, p_attn=p_attn, p=p)
    (y * G.float().to(DEV)).sum().backward()
    assert len(seeds) == (p_attn > 0) + (p > 0)
    cm = _mask((ei.shape[1], H), p_attn, seeds[0]) if p_attn > 0 else None
    om = _mask(tuple(y.shape), p, seeds[-1]) if p > 0 else None
    ref = [t.clone().requires_grad_(True) for t in (z, ze, att, bias)]
    avo, aeo = _logits(ref[0], ref[1], ref[2], n_e, H, F, attributed)
    yo = orc.propagate(ref[0], avo, aeo, ei, n_e, H, D, B, 0.2, concat, ref[3], act, cm, om, softmax_by)
    (yo * G).sum().backward()
    return y.detach().cpu().double(), yo.detach(), [t.grad for t in dev], [t.grad for t in ref], (n_v, bias, om)


@pytest.mark.parametrize("H,F,concat,act,p,p_attn,attributed,large", KERNEL_CASES)
def test_hattn_propagate_vs_oracle(monkeypatch, H, F, concat, act, p, p_attn, attributed, large):
    y, yo, gd, gr, (n_v, bias, om) = _run_kernel(monkeypatch, H, F, concat, act, p, p_attn, attributed, large)
    torch.testing.assert_close(y, yo, **TOL)
    iso = orc.act_fn(bias, act).expand(5, -1) * (om[-5:] if om is not None else 1.0)       # isolated vertices: the bias alone
    torch.testing.assert_close(y[-5:], iso, **TOL)
    gz, gze, gatt, gb = gd
    torch.testing.assert_close(gz.cpu().double(), gr[0], **_gtol(gr[0]))
    assert float(gz[-5:].abs().max()) == 0.0
    if attributed:
        torch.testing.assert_close(gze.cpu().double(), gr[1], **_gtol(gr[1]))
    else:
        assert gze is None and gr[1] is None
    torch.testing.assert_close(gatt.cpu().double(), gr[2], **PTOL)
    torch.testing.assert_close(gb.cpu().double(), gr[3], **PTOL)


def test_sabotage_softmax_axis_is_seen(monkeypatch):
    """The oracle with the softmax grouped by hyperedge instead of by vertex must FAIL the comparison the kernel passes."""
    y, yo, _, _, _ = _run_kernel(monkeypatch, 4, 16, True, None, 0.0, 0.0, False, False, softmax_by="edge")
    with pytest.raises(AssertionError):
        torch.testing.assert_close(y, yo, **TOL)


def test_backward_is_bit_stable(monkeypatch):
    """No float atomics, one summation order: two runs give identical bits."""
    a = _run_kernel(monkeypatch, 4, 16, True, "elu", 0.0, 0.0, True, False)
    b = _run_kernel(monkeypatch, 4, 16, True, "elu", 0.0, 0.0, True, False)
    assert torch.equal(a[0], b[0]) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_errors_leave_the_device_usable():
    from allset_amd import hattn_propagate, ops
    from allset_amd._lib import AllSetHipError
    n_v, ei, inc = _graph(False)
    D = torch.ones(n_v, device=DEV)
    B = torch.ones(300, device=DEV)
    z = torch.randn(n_v, 520, device=DEV)
    with pytest.raises(AllSetHipError, match="exceeds the built maximum"):
        hattn_propagate(z, torch.zeros(n_v, 1, device=DEV), torch.zeros(300, 1, device=DEV), inc, 1, D, B)
    with pytest.raises(AllSetHipError):
        hattn_propagate(z[:, :64], torch.zeros(n_v, 2, device=DEV), torch.zeros(299, 2, device=DEV), inc, 2, D, B)     # ae rows
    with pytest.raises(AllSetHipError, match="heads"):
        ops.hattn_hop(inc.by_dst, torch.ones(inc.nnz, 3, device=DEV), z[:, :64], 3, 300)                               # 3 does not divide 64
    with pytest.raises(AllSetHipError):
        hattn_propagate(z[:, :64].cpu(), torch.zeros(n_v, 2), torch.zeros(300, 2), inc, 2, D, B)
    y = hattn_propagate(z[:, :64], torch.zeros(n_v, 2, device=DEV), torch.zeros(300, 2, device=DEV), inc, 2, D, B)
    assert torch.isfinite(y).all()


# ---- layer level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in sorted(hc.CASES) if not hc.spec(n)["train"]])
def test_conv_equals_recorded_reference(name):
    """The HIP path (fp32) against what the reference's own layer computed: output, d/dx and every parameter gradient."""
    from allset_amd.baselines import HypergraphAttentionConv
    c = hc.spec(name)
    fx = hc.load(hc.FILE)
    x, ei, w = hc.inputs(c)
    torch.manual_seed(c["seed"])
    conv = HypergraphAttentionConv(hc.F_IN, c["out"], heads=c["heads"], concat=c["concat"])
    conv.load_state_dict({k: v.float() for k, v in hc.perturb(conv.state_dict(), c).items()})
    conv = conv.to(DEV).eval()
    xd = x.float().to(DEV).requires_grad_(True)
    pad = hc.N_E - (int(ei[1].max()) + 1)
    assert pad == 0
    out = conv(xd, ei.to(DEV), w.float().to(DEV) if w is not None else None)
    (out * hc.cotangent(c, out.shape[0]).float().to(DEV)).sum().backward()
    ref = lambda k: torch.from_numpy(fx[f"{name}/{k}"])
    torch.testing.assert_close(out.detach().cpu().double(), ref("out"), **TOL)
    torch.testing.assert_close(xd.grad.cpu().double(), ref("grad_x"), **_gtol(ref("grad_x")))
    for k, prm in conv.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), ref(f"grad:{k}"), msg=lambda m, k=k: f"{k}: {m}", **PTOL)


@pytest.mark.parametrize("attention,mode", [(False, None), (True, None), (True, "tensor"), (True, "mean")])
def test_conv_with_hyperedge_weight(attention, mode):
    from allset_amd.baselines import HypergraphAttentionConv, HypergraphConv
    n_v, n_e, F_in, H, C = 300, 120, 10, 2, 6
    ei = hc.hypergraph(n_v, n_e, seed=5, empty=True, isolated=3)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(n_v, F_in, generator=g, dtype=torch.float64)
    w = torch.rand(n_e, generator=g, dtype=torch.float64) + 0.5
    attr = torch.randn(n_e, F_in, generator=g, dtype=torch.float64) if mode == "tensor" else mode
    torch.manual_seed(5)
    conv = HypergraphAttentionConv(F_in, C, heads=H) if attention else HypergraphConv(F_in, C)
    with torch.no_grad():
        conv.bias.add_(0.1 * torch.randn(conv.bias.shape, generator=g))
    conv = conv.to(DEV).eval()
    xd = x.float().to(DEV).requires_grad_(True)
    ad = attr.float().to(DEV).requires_grad_(True) if mode == "tensor" else attr
    kw = dict(hyperedge_attr=ad) if attention else {}
    out = conv(xd, ei.to(DEV), w.float().to(DEV), **kw)
    G = torch.randn(out.shape, generator=g, dtype=torch.float64)
    (out * G.float().to(DEV)).sum().backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in conv.state_dict().items()}
    xo = x.clone().requires_grad_(True)
    ao = attr.clone().requires_grad_(True) if mode == "tensor" else attr
    if attention:
        oo = orc.conv(xo, sd["weight"], sd["att"], sd["bias"], ei, n_e, H, hyperedge_weight=w, hyperedge_attr=ao)
    else:
        oo = orc.plain_conv(xo, sd["weight"], sd["bias"], ei, n_e, hyperedge_weight=w)
    (oo * G).sum().backward()
    torch.testing.assert_close(out.detach().cpu().double(), oo.detach(), **TOL)
    torch.testing.assert_close(xd.grad.cpu().double(), xo.grad, **TOL)
    if mode == "tensor":
        torch.testing.assert_close(ad.grad.cpu().double(), ao.grad, **TOL)
    for k, prm in conv.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), sd[k].grad, msg=lambda m, k=k: f"{k}: {m}", **PTOL)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _args(**kw):
    a = dict(All_num_layers=2, dropout=0.5, MLP_hidden=16, num_features=24, num_classes=5, HCHA_symdegnorm=False,
             HCHA_use_attention=True, heads=4, output_heads=1, HCHA_attn_drop=0.5)
    a.update(kw)
    return SimpleNamespace(**a)


def _model_data(kw, seed=0):
    from allset_amd.baselines import HCHA
    from allset_amd.preprocessing import generate_norm_HCHA
    args = _args(**kw)
    n_v, n_e = 400, 160
    ei = hc.hypergraph(n_v, n_e, seed=seed, empty=True)
    ei = torch.cat([ei, torch.stack([torch.arange(n_v), n_e + torch.arange(n_v)])], dim=1)      # a self-loop hyperedge per vertex
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_v, args.num_features, generator=g, dtype=torch.float64)
    torch.manual_seed(seed)
    model = HCHA(args)
    for prm in model.parameters():                      # non-zero biases (the reference initialises them to zeros)
        with torch.no_grad():
            prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    data = SimpleNamespace(x=x.float().to(DEV), edge_index=ei.to(DEV), n_x=[n_v])
    generate_norm_HCHA(data, False)
    return args, model.to(DEV), data, x, ei, n_e + n_v


def _oracle(args, sd, x, ei, n_e, cm=None, om=None):
    return orc.hcha_forward(sd, x, ei, n_e, max(args.All_num_layers, 2), args.heads, args.output_heads, cm, om)


@pytest.mark.parametrize("training", [False, True])
@pytest.mark.parametrize("L,out_heads", [(1, 1), (2, 2), (3, 1)])
def test_model_vs_oracle(monkeypatch, L, out_heads, training):
    args, model, data, x, ei, n_e = _model_data(dict(All_num_layers=L, output_heads=out_heads))
    model.train(training)
    seeds = _seeds(monkeypatch)
    data.x.requires_grad_(True)
    logits = model(data)
    G = torch.randn(logits.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    (logits * G.float().to(DEV)).sum().backward()
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    cm = om = None
    if training:
        n = len(model.convs)
        assert len(seeds) == 2 * n - 1                   # per conv: the coefficient's mask, then (all but the last) the output's
        heads = [args.heads] * (n - 1) + [out_heads]
        cm = [_mask((ei.shape[1], heads[i]), args.HCHA_attn_drop, seeds[2 * i]) for i in range(n)]
        om = [_mask((x.shape[0], args.heads * args.MLP_hidden), args.dropout, seeds[2 * i + 1]) for i in range(n - 1)]
    xo = x.clone().requires_grad_(True)
    lo = _oracle(args, sd, xo, ei, n_e, cm, om)
    (lo * G).sum().backward()
    torch.testing.assert_close(logits.detach().cpu().double(), lo.detach(), **TOL)
    torch.testing.assert_close(data.x.grad.cpu().double(), xo.grad, **TOL)
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), sd[k].grad, msg=lambda m, k=k: f"{k}: {m}", **PTOL)


# ---- graphs and training -------------------------------------------------------------------------------------------------------
def test_graphed_train_step_equals_eager():
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    args, model, data, x, ei, n_e = _model_data({})
    y = torch.randint(0, args.num_classes, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    opt_e = FusedAdam(eager.parameters(), lr=0.01)
    eager.eval()                                          # dropout off: the graphed step below runs train_mode=False
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


def test_graphed_training_mode_step_equals_eager(monkeypatch):
    """Both dropouts live: one replay of the captured step equals one eager step that draws its masks from the same device seed
    counter value and the same per-site salts."""
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    args, model, data, x, ei, n_e = _model_data({})
    y = torch.randint(0, args.num_classes, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    salts = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: salts.append(real()) or salts[-1])
    step = GraphedTrainStep(model, data, loss_fn, FusedAdam(model.parameters(), lr=0.01), warmup=3)
    n_sites = len(salts) // 4                                 # three warm-up steps and the captured one
    assert n_sites == 2 * len(model.convs) - 1
    captured = salts[-n_sites:]
    counter = step.counter.clone()
    loss_g = step().clone()
    torch.cuda.synchronize()
    assert not torch.equal(step.counter, counter)
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


def test_adam_trajectory_follows_oracle():
    from allset_amd.optim import FusedAdam
    args, model, data, x, ei, n_e = _model_data({})
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
        torch.nn.functional.cross_entropy(_oracle(args, sd, x, ei, n_e), y).backward()
        opt_o.step()
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.detach().cpu().double(), sd[k].detach(), rtol=1e-3, atol=1e-4, msg=lambda m, k=k: f"{k}: {m}")


def test_train_driver_end_to_end(tmp_path):
    cmd = [sys.executable, "-m", "allset_amd.train", "--dname", "synthetic", "--method", "HCHA", "--HCHA_use_attention", "--heads", "2",
           "--epochs", "5", "--runs", "1", "--hip_graph", "1", "--res_root", str(tmp_path)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout
