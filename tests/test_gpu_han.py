"""GPU: the HAN baseline -- the attention hop (csrc/han.hip, functional.han_gat_propagate) forward and backward against the float64
restatement of tests/han_oracle.py on random multigraphs (duplicate edges, doubled loops, long rows), with the product's own
attention-dropout factors read back through functional.han_edge_keep and fed to the restatement; the semantic attention forward and
backward; the whole model's logits, d/dx and every parameter gradient on the cases of tests/han_cases.py in eval mode and in training
mode (product masks) at the suite's fp32 parity level, rtol = atol = 1e-4; the stacked strided write against separate outputs, bit
for bit; run-to-run bit-identity; a 30-epoch synthetic run through the driver.

The leaky-relu kink: fp32 and float64 may disagree on the side of a pre-activation ``el[s] + er[t]`` only where it is within fp32
rounding of 0.  Every comparison asserts, from the float64 restatement alone, that the nearest pre-activation is more than 1e-5 away;
the seeds were fixed on the CPU so that it is.  ELU with alpha = 1 has a continuous derivative and needs no guard."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_cases as hc  # noqa: E402
import han_oracle as orc  # noqa: E402

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


# ---- kernel level --------------------------------------------------------------------------------------------------------------
N_HOP = 1500
# (heads, channels, attention dropout, long rows, seed): the seed is the first of 0, 1, 2, ... whose inputs keep every pre-activation
# 1e-5 away from 0 (found with hop_inputs and the restatement alone, on the CPU)
HOP_CASES = [(1, 1, 0.0, (), 0), (1, 7, 0.6, (70,), 0), (2, 3, 0.0, (1200,), 0), (2, 8, 0.5, (), 0), (8, 8, 0.6, (70, 1300), 3),
             (8, 8, 0.0, (), 3), (4, 32, 0.6, (1100,), 0), (8, 64, 0.5, (65,), 1), (1, 128, 0.6, (), 0),
             (16, 5, 0.6, (70,), 0)]          # (C % 4 != 0 with a row wider than 64: heads straddle the source pass's lane chunks)


def hop_inputs(H, C, long_rows, seed, n=N_HOP):
    """A random directed multigraph over ``n`` ids: 5 n random edges, 200 of them listed twice, a self-loop on every node (every row
    non-empty) and a second one on every third, rows of the given lengths; fp32-representable float64 inputs."""
    rng = np.random.default_rng(2000 * seed + 17 * H + C)
    src, dst = rng.integers(0, n, size=5 * n), rng.integers(0, n, size=5 * n)
    src, dst = np.concatenate([src, src[:200], np.arange(n), np.arange(0, n, 3)]), np.concatenate([dst, dst[:200], np.arange(n), np.arange(0, n, 3)])
    for i, L in enumerate(long_rows):
        src, dst = np.concatenate([src, rng.integers(0, n, size=L)]), np.concatenate([dst, np.full(L, i)])
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    return torch.from_numpy(src.astype(np.int64)), torch.from_numpy(dst.astype(np.int64)), f(n, H * C), f(n, H), f(n, H), f(H * C), f(n, H * C)


@pytest.mark.parametrize("case", HOP_CASES, ids=lambda c: f"H{c[0]}C{c[1]}-p{c[2]}-long{len(c[3])}")
def test_hop_vs_float64(monkeypatch, case):
    from allset_amd.functional import han_edge_keep, han_gat_propagate
    from allset_amd.han import MetapathGraph
    H, C, p, long_rows, seed = case
    n = N_HOP
    src, dst, x, el, er, b, G = hop_inputs(H, C, long_rows, seed)
    graph = MetapathGraph(src.to(DEV), dst.to(DEV), n)
    seeds = _capture_seeds(monkeypatch)
    dv = [t.float().to(DEV).requires_grad_(True) for t in (x, el, er, b)]
    y = han_gat_propagate(dv[0], dv[1], dv[2], graph, H, 0.2, dv[3], p)
    (y * G.float().to(DEV)).sum().backward()
    keep = None
    if p > 0:
        assert len(seeds) == 1
        keep = han_edge_keep(graph, H, p, seeds[0]).cpu().double()
        assert set(keep.unique().tolist()) == {0.0, float(np.float32(1) / (np.float32(1) - np.float32(p)))}
        assert abs(float((keep > 0).double().mean()) - (1 - p)) < 0.03
    leaves = [t.clone().requires_grad_(True) for t in (x, el, er, b)]
    rep = []
    yo = orc.gat_hop(src, dst, n, leaves[0], leaves[1], leaves[2], leaves[3], keep, rep)
    (yo * G).sum().backward()
    print(f"min |el[s] + er[t]| = {rep[0]:.3e}")
    assert rep[0] > hc.KINK_MARGIN
    deg = torch.bincount(dst, minlength=n)
    assert int(deg.min()) >= 1 and (not long_rows or int(deg.max()) >= max(long_rows))
    _close(y, yo, "y")
    for got, want, what in zip(dv, leaves, ("gx", "gel", "ger", "gbias")):
        _close(got.grad, want.grad, what)


def test_hop_cases_cover_the_kernel_paths():
    assert {c[0] for c in HOP_CASES} >= {1, 2, 8}
    assert any(c[3] and max(c[3]) > 1024 for c in HOP_CASES) and any(c[3] and 64 < min(c[3]) <= 1024 for c in HOP_CASES)
    assert any(c[1] % 4 for c in HOP_CASES) and any(c[0] * c[1] == 512 for c in HOP_CASES)
    assert any(c[1] % 4 and c[0] * c[1] > 64 for c in HOP_CASES)
    assert any(c[2] == 0.5 for c in HOP_CASES) and any(c[2] == 0.6 for c in HOP_CASES)      # both resolutions of the hash mask


def test_zero_in_degree_and_unbuilt_shapes_are_errors():
    from allset_amd import _lib
    from allset_amd.functional import han_gat_propagate, semantic_attention
    from allset_amd.han import MetapathGraph
    with pytest.raises(ValueError, match="0-in-degree"):
        MetapathGraph(torch.tensor([0, 1], device=DEV), torch.tensor([1, 1], device=DEV), 2)
    g = MetapathGraph(torch.arange(4, device=DEV), torch.arange(4, device=DEV), 4)
    with pytest.raises(_lib.AllSetHipError, match="exceeds the built maximum"):
        han_gat_propagate(torch.zeros(4, 1024, device=DEV), torch.zeros(4, 2, device=DEV), torch.zeros(4, 2, device=DEV), g, 2)
    leaf = torch.zeros(4, 8, device=DEV, requires_grad=True)
    with pytest.raises(ValueError, match="out must be a buffer"):
        han_gat_propagate(torch.zeros(4, 8, device=DEV), torch.zeros(4, 2, device=DEV), torch.zeros(4, 2, device=DEV), g, 2, out=leaf * 1.0)
    with pytest.raises(_lib.AllSetHipError, match="built for hidden"):
        semantic_attention(torch.zeros(4, 2, 256, device=DEV), torch.zeros(128, 256, device=DEV), torch.zeros(128, device=DEV),
                           torch.zeros(128, device=DEV))


@pytest.mark.parametrize("N,M,D", [(300, 2, 64), (1000, 3, 8), (77, 1, 128), (513, 2, 20), (5000, 2, 64), (4100, 5, 100)])
def test_semantic_attention_vs_float64(N, M, D):
    from allset_amd.functional import semantic_attention
    g = torch.Generator().manual_seed(N + D)
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    z, W1, b1, w2, G = f(N, M, D), f(128, D) / np.sqrt(D), f(128), f(1, 128), f(N, D)
    w2 = w2 * 3                                                          # (so that beta is far from uniform)
    dv = [t.float().to(DEV).requires_grad_(True) for t in (z, W1, b1, w2)]
    out = semantic_attention(dv[0], dv[1], dv[2], dv[3].view(-1))
    (out * G.float().to(DEV)).sum().backward()
    leaves = [t.clone().requires_grad_(True) for t in (z, W1, b1, w2)]
    oo = orc.semantic_attention(*leaves)
    (oo * G).sum().backward()
    _close(out, oo, "out")
    for got, want, what in zip(dv, leaves, ("gz", "gW1", "gb1", "gq")):
        _close(got.grad, want.grad, what)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _model_and_data(name):
    from allset_amd.han import HAN, metapath_graphs
    c = hc.spec(name)
    x, pairs, n_v, n_e = hc.raw_data(c)
    data = SimpleNamespace(edge_index=torch.from_numpy(pairs).to(DEV), n_x=[n_v], num_hyperedges=[n_e])
    gs = metapath_graphs(data)
    want = hc.dense_metapath_edges(pairs, n_v, n_e)
    for g, (r, cc) in zip(gs, want):
        assert np.array_equal(g.src.cpu().numpy(), r) and np.array_equal(g.dst.cpu().numpy(), cc)
    torch.manual_seed(c["seed"])
    model = HAN(num_meta_paths=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=hc.DROPOUT)
    sd64 = hc.perturb(model.state_dict(), c)
    model.load_state_dict({k: v.float() for k, v in sd64.items()})
    sd64 = {k: v.detach().double() for k, v in model.state_dict().items()}               # the fp32 values the device model holds
    return c, model.to(DEV), gs, x, sd64, [(torch.from_numpy(r), torch.from_numpy(cc)) for r, cc in want]


# training mode: ``torch.manual_seed(MASK_SEED[name])`` before the forward fixes the product's dropout seeds; the value is the first of
# 0, 1, 2, ... under which the RESTATEMENT, fed the resulting masks, keeps every pre-activation 1e-5 away from 0 (a node whose 12 input
# features are all dropped has el = er = 0 exactly and puts its own self-loop on the kink).  Chosen from the restatement's margin alone.
MASK_SEED = {name: 1 for name in hc.CASES}            # (seed 0 drops all 12 features of one node in every case)


def _run_model(monkeypatch, name, training):
    from allset_amd import dense
    from allset_amd.functional import han_edge_keep
    c, model, gs, x, sd64, edges = _model_and_data(name)
    n = x.shape[0]
    model.train(training)
    seeds = _capture_seeds(monkeypatch)
    if training:
        torch.manual_seed(MASK_SEED[name])
    xd = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
    logits = model(gs, xd)
    G = torch.from_numpy(hc.cotangent(c, n))
    (logits * G.float().to(DEV)).sum().backward()
    masks = None
    if training:
        assert len(seeds) == 4 * len(c["heads"])                        # per conv: the feature mask, then the attention mask
        masks, k = [], 0
        for l, H in enumerate(c["heads"]):
            width = c["F"] if l == 0 else c["hidden"] * c["heads"][l - 1]
            layer = []
            for g in gs:
                fk = dense.dropout_scale((n, width), hc.DROPOUT, seeds[k], DEV).cpu().double()
                ek = han_edge_keep(g, H, hc.DROPOUT, seeds[k + 1]).cpu().double()
                layer.append((fk, ek))
                k += 2
            masks.append(layer)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = torch.from_numpy(x).float().double().requires_grad_(True)
    report = []
    lo = orc.han_forward(sd, edges, n, xo, len(c["heads"]), masks, report)
    (lo * G).sum().backward()
    print(f"{name} training={training}: kink margin {min(report):.3e}")
    assert min(report) > hc.KINK_MARGIN
    _close(logits, lo, "logits")
    _close(xd.grad, xo.grad, "grad_x")
    for k, prm in model.named_parameters():
        _close(prm.grad, sd[k].grad, f"grad:{k}")


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_model_eval_vs_oracle(monkeypatch, name):
    _run_model(monkeypatch, name, training=False)


@pytest.mark.parametrize("name", sorted(n for n in hc.CASES if not n.startswith("cora")))
def test_model_training_vs_oracle_with_product_masks(monkeypatch, name):
    _run_model(monkeypatch, name, training=True)


def test_stacked_write_equals_separate_outputs_bitwise():
    from allset_amd.functional import han_gat_propagate
    from allset_amd.han import MetapathGraph
    H, C, n = 8, 8, N_HOP
    d = H * C
    gs, ins = [], []
    for seed in (0, 1, 2):
        src, dst, x, el, er, b, _ = hop_inputs(H, C, (70,), seed)
        gs.append(MetapathGraph(src.to(DEV), dst.to(DEV), n))
        ins.append([t.float().to(DEV) for t in (x, el, er, b)])
    z = torch.full((n, 3 * d), float("nan"), device=DEV)
    for i, (g, (x, el, er, b)) in enumerate(zip(gs, ins)):
        z = han_gat_propagate(x, el, er, g, H, 0.2, b, 0.0, out=z, block=i)
    sep = [han_gat_propagate(x, el, er, g, H, 0.2, b, 0.0) for g, (x, el, er, b) in zip(gs, ins)]
    assert torch.equal(z.view(n, 3, d), torch.stack(sep, dim=1))


def test_two_identical_runs_are_bit_identical():
    c, model, gs, x, _, _ = _model_and_data("han_h8_h2_train")
    model.train()
    outs = []
    for _ in range(2):
        torch.manual_seed(11)
        model.zero_grad(set_to_none=True)
        xd = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
        logits = model(gs, xd)
        logits.square().sum().backward()
        outs.append([logits.detach().clone(), xd.grad.clone()] + [p.grad.clone() for p in model.parameters()])
    for a, b in zip(*outs):
        assert torch.equal(a, b)


def test_driver_lowers_the_training_loss_in_30_epochs(capsys):
    from allset_amd import han
    args = han.setup(han.build_parser().parse_args(["--dataset", "synthetic", "--runs", "1", "--num_epochs", "30"]).__dict__)
    hist = han.main(args)
    losses = hist["train_loss"][0]
    out = capsys.readouterr().out
    print(f"train loss: first {losses[0]:.4f}, last {losses[-1]:.4f}; test acc {hist['acc'][0]:.2f}")
    assert len(losses) == 30 and losses[-1] < losses[0]
    assert ">> Final test acc:" in out and "test marco f1:" in out and ">> Train time per run:" in out
