"""HyperGCN on the MI355X (csrc/hypergcn.hip behind functional.hypergcn_structure / hypergcn_propagate and baselines.HyperGCN).

Kernel level: the extremes S / I of every case and both mediator modes equal the float64 restatement's exactly (integer comparison; the
cases keep hypergcn_cases.GAP_MARGIN, asserted on the CPU in tests/test_hypergcn_reference.py), ``dinv`` and the hop follow it at the
1e-4 fp32 parity of the GPU suite; every built width and one that is not; fused against the composition; skewed hyperedge sizes through
both E->V variants; a role-swapped structure must FAIL the same comparison.  Model level: logits and every gradient against the recorded
reference in eval mode and, in training mode, with the product's own hash masks fed to the restatement; the re-approximating forward
captured as a graph and replayed with a changed projection vector; the driver end to end in both fast settings."""
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hypergcn_cases as hc  # noqa: E402
import hypergcn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
FILE_OF = {name: file for file, names in hc.FILES.items() for name in names}


def _close(got, want, what, tol=1e-4):
    want = torch.as_tensor(want).detach().double()
    got = got.detach().cpu().double()
    print(f"{what}: max |diff| {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got, want, rtol=tol, atol=tol * max(1.0, float(want.abs().max())), msg=lambda m: f"{what}: {m}")


def _incidence(pairs, n_v, n_e):
    from allset_amd.incidence import Incidence
    return Incidence.from_edge_index(torch.from_numpy(pairs).to(DEV).contiguous(), n_src=n_v, n_dst=n_e)


def _structure(z32, rv32, pairs, n_v, n_e, med):
    from allset_amd.functional import hypergcn_structure
    return hypergcn_structure(z32.to(DEV), rv32.to(DEV), _incidence(pairs, n_v, n_e), med)


MODES = [(name, med) for name in hc.CASES for med in (True, False) if med is False or not hc.spec(name)["singletons"]]


@pytest.mark.parametrize("name,med", MODES)
def test_structure_and_hop_match_restatement(name, med):
    """S, I exactly; dinv and A x (no epilogue, d = 16) at fp32 parity."""
    from allset_amd.functional import hypergcn_propagate
    c = hc.spec(name)
    x, pairs, n_v, n_e = hc.raw_data(c)
    members = hc.member_lists(pairs, n_e)
    g = torch.Generator().manual_seed(c["seed"])
    # Z = the case's input with the recorded projection vector of the reference where the case is fast (its gaps: asserted on the
    # CPU), else with a seeded one; the small cases add a random [n, 16] matrix standing for a hidden layer's H W
    rv_x = torch.from_numpy(hc.load(FILE_OF[name])[f"{name}/rv0"]).float() if c["fast"] else torch.rand(c["F"], generator=g)
    zs = [(torch.from_numpy(x).float(), rv_x)]
    if not c["ties"] and n_v <= 100:
        zs.append((torch.randn(n_v, 16, generator=g), torch.rand(16, generator=g)))
    for z32, rv32 in zs:
        S, I, gaps = orc.roles(z32.double().numpy(), rv32.double().numpy(), members)
        rel = [min(a, b) / s for a, b, s in (t for t in gaps if t is not None) if min(a, b) > 0]
        print(f"{name} med={med} width {z32.shape[1]}: smallest relative projection gap {min(rel):.3e}")
        assert min(rel) > hc.GAP_MARGIN                      # (of THIS test's own draw; the cases' draws: test_hypergcn_reference.py)
        st = _structure(z32, rv32, pairs, n_v, n_e, med)
        np.testing.assert_array_equal(st.S.cpu().numpy(), S)
        np.testing.assert_array_equal(st.I.cpu().numpy(), I)
        np.testing.assert_array_equal(st.size.cpu().numpy(), np.array([len(m) for m in members]))
        A, dinv = orc.dense_A(n_v, members, S, I, med)
        _close(st.dinv, dinv, "dinv", 1e-5)
        h = torch.randn(n_v, 16, generator=g)
        _close(hypergcn_propagate(h.to(DEV), st, fused=True), A @ h.double().numpy(), "A x")


def _small(med, seed=3, n_v=500, n_e=260, big=()):
    """A hypergraph of 2..8-member hyperedges plus the sizes in ``big``; returns (pairs, members, n_v, n_e)."""
    rng = np.random.default_rng(seed)
    members = [[int(v) for v in rng.choice(n_v - 5, size=int(rng.integers(2, 9)), replace=False)] for _ in range(n_e - len(big))]
    members += [[int(v) for v in rng.choice(n_v - 5, size=k, replace=False)] for k in big]
    v = np.array([m for mem in members for m in mem], dtype=np.int64)
    e = np.array([i for i, mem in enumerate(members) for _ in mem], dtype=np.int64)
    order = rng.permutation(v.size)
    return np.stack([v[order], e[order]]), members, n_v, len(members)


def _oracle_hop(st_args, h, bias=None, relu=False):
    n_v, members, S, I, med = st_args
    out = orc.sparse_apply(n_v, orc.triplets(members, S, I, med), h.double().numpy())
    if bias is not None:
        out = out + bias.double().numpy()
    return np.maximum(out, 0.0) if relu else out


@pytest.mark.parametrize("med", [True, False])
@pytest.mark.parametrize("d", [8, 16, 32, 64, 128, 256, 3, 5, 7, 40, 12, 100])
def test_every_built_width(d, med):
    """The widths the width rule produces (powers of two 8..256), class counts of the last layer, and two more multiples of 4; with the
    bias + relu epilogue and the gradient in x and bias (the hop applied to the masked cotangent)."""
    from allset_amd import ops
    from allset_amd.functional import hypergcn_propagate
    pairs, members, n_v, n_e = _small(med)
    g = torch.Generator().manual_seed(d)
    z32, rv32 = torch.randn(n_v, 16, generator=g), torch.rand(16, generator=g)
    S, I, _ = orc.roles(z32.double().numpy(), rv32.double().numpy(), members)
    st = _structure(z32, rv32, pairs, n_v, n_e, med)
    np.testing.assert_array_equal(st.S.cpu().numpy(), S)
    np.testing.assert_array_equal(st.I.cpu().numpy(), I)
    h = torch.randn(n_v, d, generator=g)
    bias = torch.randn(d, generator=g)
    hd = h.to(DEV).requires_grad_(True)
    bd = bias.to(DEV).requires_grad_(True)
    assert ops.hypergcn_hop_supported(hd)
    y = hypergcn_propagate(hd, st, bd, act="relu", fused=True)
    want = _oracle_hop((n_v, members, S, I, med), h, bias, relu=True)
    _close(y, want, f"hop d={d}")
    G = torch.randn(n_v, d, generator=g)
    (y * G.to(DEV)).sum().backward()
    gm = G.double() * torch.from_numpy(want > 0).double()
    _close(hd.grad, _oracle_hop((n_v, members, S, I, med), gm), f"grad x d={d}")
    _close(bd.grad, gm.sum(0), f"grad bias d={d}")


@pytest.mark.parametrize("med", [True, False])
@pytest.mark.parametrize("d", [70, 260, 512])
def test_unbuilt_width_is_an_error_for_the_kernel_and_composed_in_python(d, med):
    from allset_amd import ops
    from allset_amd._lib import AllSetHipError
    from allset_amd.functional import hypergcn_propagate
    pairs, members, n_v, n_e = _small(med)
    g = torch.Generator().manual_seed(d)
    z32, rv32 = torch.randn(n_v, 16, generator=g), torch.rand(16, generator=g)
    S, I, _ = orc.roles(z32.double().numpy(), rv32.double().numpy(), members)
    st = _structure(z32, rv32, pairs, n_v, n_e, med)
    h = torch.randn(n_v, d, generator=g)
    bias = torch.randn(d, generator=g)
    assert not ops.hypergcn_hop_supported(h.to(DEV))
    with pytest.raises(AllSetHipError, match="not built"):
        hypergcn_propagate(h.to(DEV), st, fused=True)
    hd = h.to(DEV).requires_grad_(True)
    y = hypergcn_propagate(hd, st, bias.to(DEV), act="relu")
    want = _oracle_hop((n_v, members, S, I, med), h, bias, relu=True)
    _close(y, want, f"composed hop d={d}")
    G = torch.randn(n_v, d, generator=g)
    (y * G.to(DEV)).sum().backward()
    _close(hd.grad, _oracle_hop((n_v, members, S, I, med), G.double() * torch.from_numpy(want > 0).double()), f"composed grad d={d}")


@pytest.mark.parametrize("med", [True, False])
@pytest.mark.parametrize("d,p", [(16, 0.5), (64, 0.5), (7, 0.5), (64, 0.3)], ids=["16", "64", "7", "64-p0.3"])
def test_fused_equals_composed_with_dropout(d, p, med, monkeypatch):
    """Same seed, same mask convention: the two-launch hop and the composition from hconv launches agree, dropout included."""
    from allset_amd import dense
    from allset_amd.functional import hypergcn_propagate
    pairs, members, n_v, n_e = _small(med, seed=5)
    g = torch.Generator().manual_seed(d)
    st = _structure(torch.randn(n_v, 16, generator=g), torch.rand(16, generator=g), pairs, n_v, n_e, med)
    h, bias, G = torch.randn(n_v, d, generator=g).to(DEV), torch.randn(d, generator=g).to(DEV), torch.randn(n_v, d, generator=g).to(DEV)
    monkeypatch.setattr(dense, "_draw_seed", lambda: 1234567)
    outs = []
    for fused in (True, False):
        hd = h.clone().requires_grad_(True)
        y = hypergcn_propagate(hd, st, bias, act="relu", p=p, fused=fused)
        (y * G).sum().backward()
        outs.append((y.detach(), hd.grad))
    frac = float((outs[0][0] == 0).float().mean())
    assert abs(frac - (1.0 - 0.5 * (1.0 - p))) < 0.15, frac            # relu (half) and p together: (0.6, 0.9) at p = 0.5
    assert torch.equal(outs[0][0] == 0, outs[1][0] == 0)
    _close(outs[0][0], outs[1][0].cpu(), "fused vs composed", 1e-5)
    _close(outs[0][1], outs[1][1].cpu(), "fused vs composed grad", 1e-5)


@pytest.mark.parametrize("med", [True, False])
@pytest.mark.parametrize("variant", [1, 2, None])
def test_skewed_hyperedge_sizes(variant, med):
    """Two hyperedges of 3000 and 700 members among 6000 small ones over 20000 vertices: the hyperedge-major CSR gets a row order, the
    E->V pass runs as one wavefront per row (1), as the short-row kernel (2) and as the library chooses."""
    from allset_amd.functional import hypergcn_propagate
    pairs, members, n_v, n_e = _small(med, seed=11, n_v=20000, n_e=6002, big=(3000, 700))
    g = torch.Generator().manual_seed(1)
    z32, rv32 = torch.randn(n_v, 16, generator=g), torch.rand(16, generator=g)
    S, I, _ = orc.roles(z32.double().numpy(), rv32.double().numpy(), members)
    st = _structure(z32, rv32, pairs, n_v, n_e, med)
    assert st.inc.by_dst.row_order is not None
    np.testing.assert_array_equal(st.S.cpu().numpy(), S)
    np.testing.assert_array_equal(st.I.cpu().numpy(), I)
    h = torch.randn(n_v, 32, generator=g)
    y = hypergcn_propagate(h.to(DEV), st, act="relu", variant=variant, fused=True)
    _close(y, _oracle_hop((n_v, members, S, I, med), h, relu=True), f"variant {variant}")


def test_role_swapped_structure_fails_the_comparison():
    """The comparison can tell: with the extreme / mediator rows of the per-hyperedge buffer exchanged (colx ^ 1), or with S and I of
    the restatement exchanged for an asymmetric check of dinv-free sums, the same assertion fails."""
    from allset_amd.functional import hypergcn_propagate
    pairs, members, n_v, n_e = _small(True)
    g = torch.Generator().manual_seed(0)
    z32, rv32 = torch.randn(n_v, 16, generator=g), torch.rand(16, generator=g)
    S, I, _ = orc.roles(z32.double().numpy(), rv32.double().numpy(), members)
    st = _structure(z32, rv32, pairs, n_v, n_e, True)
    h = torch.randn(n_v, 16, generator=g)
    want = _oracle_hop((n_v, members, S, I, True), h)
    _close(hypergcn_propagate(h.to(DEV), st, fused=True), want, "intact")
    st.colx = st.colx ^ 1
    with pytest.raises(AssertionError):
        _close(hypergcn_propagate(h.to(DEV), st, fused=True), want, "swapped")


# ---- model level ------------------------------------------------------------------------------------------------------------------
def _model(c, pairs, n_v):
    from allset_amd.baselines import HyperGCN
    torch.manual_seed(c["seed"])
    model = HyperGCN(n_v, torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], hc.args_of(c))
    model.load_state_dict({k: v.float() for k, v in hc.perturb(model.state_dict(), c).items()})
    return model.to(DEV)


def _run_model(model, c, x, rvs):
    dd = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV).requires_grad_(True))
    rv32 = [torch.from_numpy(np.asarray(r)).float().to(DEV) for r in rvs]
    if c["fast"]:
        model.build_structure(dd.x.detach(), rv32[0])
        logits = model(dd)
    else:
        logits = model(dd, rv=rv32)
    G = torch.from_numpy(hc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()
    return dd, logits, G


@pytest.mark.parametrize("name", [n for n in hc.CASES if not hc.spec(n)["train"]])
def test_eval_mode_against_recorded_reference(name):
    """The product (HIP kernels, fp32) with the reference's recorded projection vectors against its recorded logits and gradients."""
    c = hc.spec(name)
    fx = hc.load(FILE_OF[name])
    x, pairs, n_v, n_e = hc.raw_data(c)
    rvs = [fx[f"{name}/rv{i}"] for i in range(len(hc.rv_sizes(c)))]
    model = _model(c, pairs, n_v).eval()
    dd, logits, _ = _run_model(model, c, x, rvs)

    def scale(k):
        kind, v = hc.result(fx, name, k)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    hc.assert_result(logits, fx, name, "logits", rtol=1e-4, atol=1e-4 * scale("logits"))
    hc.assert_result(dd.x.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"))
    for k, p in model.named_parameters():
        hc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"))


@pytest.mark.parametrize("name", [n for n in hc.CASES if hc.spec(n)["train"]])
def test_training_mode_with_product_masks(name, monkeypatch):
    """Training mode: the product's own hash masks (rebuilt from the seeds it drew) fed to the restatement, which
    tests/test_hypergcn_reference.py ties to the recorded training-mode results under explicit masks."""
    from allset_amd import dense
    c = hc.spec(name)
    fx = hc.load(FILE_OF[name])
    x, pairs, n_v, n_e = hc.raw_data(c)
    members = hc.member_lists(pairs, n_e)
    rvs = [fx[f"{name}/rv{i}"] for i in range(len(hc.rv_sizes(c)))]
    model = _model(c, pairs, n_v).train()
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    dd, logits, G = _run_model(model, c, x, rvs)
    assert len(seeds) == c["L"] - 1
    masks = [dense.dropout_scale((n_v, w), hc.DROPOUT, s, DEV).cpu().double() for w, s in zip(hc.widths(c)[1:-1], seeds)]
    assert 0.4 < float((masks[0] > 0).double().mean()) < 0.6
    sd = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    xo = torch.from_numpy(x).float().double().requires_grad_(True)
    rv64 = [np.asarray(r, dtype=np.float32).astype(np.float64) for r in rvs]
    margins, gaps = [], []
    lo = orc.forward(sd, xo, members, n_v, c["L"], c["fast"], c["med"], rv64, masks, True, margins, gaps)
    rel = [min(a, b) / s for g in gaps for a, b, s in (t for t in g if t is not None) if min(a, b) > 0]
    print(f"{name}: relu margins {['%.2e' % m for m in margins]}, smallest relative projection gap {min(rel):.3e}")
    assert min(margins) > hc.RELU_MARGIN and min(rel) > hc.GAP_MARGIN
    (lo * G).sum().backward()
    _close(logits, lo, "logits")
    _close(dd.x.grad, xo.grad, "grad_x")
    for k, p in model.named_parameters():
        _close(p.grad, sd[k].grad, f"grad:{k}")


def test_reapproximating_forward_replays_as_a_graph_with_fresh_projections():
    """No host synchronisation in the re-approximating forward: it is captured by torch.cuda.graph; the projection vectors are
    refreshed OUTSIDE the capture (in place) and every replay equals the eager forward with the same vectors."""
    c = hc.spec("hg_L3_slow_med_train")
    x, pairs, n_v, n_e = hc.raw_data(c)
    model = _model(c, pairs, n_v).eval()
    data = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV))
    model.seed_projections(5)
    with torch.no_grad():
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                model(data)
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(data)
        seen = []
        for _ in range(3):
            model.refresh_projections()
            rvs = [layer.rv.clone() for layer in model.layers]
            graph.replay()
            got = out.clone()
            want = model(data, rv=rvs)
            torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-6)
            seen.append(got)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])       # the vectors did change the result


def test_fast_structure_is_built_once_and_projections_are_seedable():
    c = hc.spec("hg_L2_fast_med")
    x, pairs, n_v, n_e = hc.raw_data(c)
    data = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV))
    outs = []
    for seed in (1, 1, 2):
        model = _model(c, pairs, n_v).eval()
        model.seed_projections(seed)
        with torch.no_grad():
            a = model(data)
            st = model.structure
            b = model(data)
        assert model.structure is st and torch.equal(a, b)
        outs.append((st.S.clone(), a))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert not torch.equal(outs[0][0], outs[2][0])


@pytest.mark.parametrize("extra", [[], ["--no-HyperGCN_fast"], ["--no-HyperGCN_fast", "--no-HyperGCN_mediators", "--hip_graph", "0"],
                                   ["--no-HyperGCN_mediators", "--All_num_layers", "3"]])
def test_train_driver_end_to_end(tmp_path, extra):
    cmd = [sys.executable, "-m", "allset_amd.train", "--method", "HyperGCN", "--dname", "synthetic", "--epochs", "8", "--runs", "1",
           "--display_step", "1", "--seed", "0", "--res_root", str(tmp_path)] + (extra if "--hip_graph" in extra else extra + ["--hip_graph", "1"])
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    losses = [float(line.split("Train Loss:")[1].split(",")[0]) for line in res.stdout.splitlines() if "Train Loss:" in line]
    assert len(losses) == 8 and all(np.isfinite(losses)), losses
    assert "All done" in res.stdout
