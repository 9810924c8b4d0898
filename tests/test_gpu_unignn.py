"""GPU: the UniGNN baselines.  Kernel level: the fused E->V hop (csrc/unignn.hip, functional.unignn_hop) and UniGAT's V->E hop with
the attention logit (functional.unigat_edge) against the float64 restatement of tests/unignn_oracle.py over both width classes
(<= 256, 260 .. 512), the short-row variant, the unfused fallback at d = 6 and d = 520 (and the raw entry points' "not built" status),
empty rows and rows longer than 64; the row-norm scale as a constant of the backward; the self term in front of the norm; the
gradient of UniGIN's eps and a replayed graph that follows it.  Model level: the product against the REFERENCE's recorded eval-mode
results (tests/golden/baselines_unignn*.npz) in both arithmetic modes of the dense tail, training mode against the restatement fed the
product's own hash masks, a graphed training step against the eager one, the train.py driver for the five methods.

Tolerance: the project's parity tolerance, rtol 1e-4 and atol 1e-4 * max(1, max |want|).  The relu / leaky-relu kinks: every recorded
case keeps RELU_MARGIN clear of them in the float64 restatement (tests/test_unignn_reference.py asserts it a priori)."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unignn_cases as gc  # noqa: E402
import unignn_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")


def _close(got, want, what):
    want = want.detach()
    got = got.detach().cpu().double().reshape(want.shape)
    print(f"{what}: max |diff| {float((got - want).abs().max()):.3e}, max |want| {float(want.abs().max()):.3e}")
    torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * max(1.0, float(want.abs().max())), msg=lambda m: f"{what}: {m}")


def _fails(got, want):
    want = want.detach()
    got = got.detach().cpu().double().reshape(want.shape)
    tol = 1e-4 * max(1.0, float(want.abs().max())) + 1e-4 * want.abs()
    return bool(((got - want).abs() > tol).any())


def hop_inputs(d, long_rows, n, per_row, seed=0):
    """Random (vertex, hyperedge) incidences over ``n`` vertices and ``n`` hyperedges with empty rows on both sides and rows of the given
    lengths; fp32-representable float64 inputs."""
    rng = np.random.default_rng(1000 * seed + d)
    V = rng.integers(0, n, size=per_row * n)
    E = rng.integers(0, n, size=per_row * n)
    keep = ((V % 13) != 5) & ((E % 11) != 3)
    V, E = V[keep], E[keep]
    for i, L in enumerate(long_rows):
        V = np.concatenate([V, np.full(L, i), rng.integers(0, n, size=L)])
        E = np.concatenate([E, rng.integers(0, n, size=L), np.full(L, i)])
    g = torch.Generator().manual_seed(seed)
    f = lambda *shape: torch.randn(*shape, generator=g, dtype=torch.float32).double()
    s = (0.2 + torch.rand(n, generator=g, dtype=torch.float32)).double()
    return torch.from_numpy(V.astype(np.int64)), torch.from_numpy(E.astype(np.int64)), f(n, d), f(n, d), s, f(n, d)


# (width, use_norm, s, self term: None / a float / 'tensor', act, p, long rows, variant, vertices, incidences per vertex)
HOP_CASES = [(4, True, True, None, None, 0.0, (), None, 2500, 6), (12, False, False, 1.0, "relu", 0.0, (70,), None, 2500, 6),
             (64, True, True, "tensor", "relu", 0.5, (70, 1500), None, 2500, 6), (128, True, False, "tensor", None, 0.0, (1100,), None, 2500, 6),
             (256, False, True, 1.0, "relu", 0.2, (65,), None, 2500, 6), (512, True, True, "tensor", "relu", 0.5, (70, 1500), None, 2500, 6),
             (320, True, False, 1.0, None, 0.0, (70,), None, 2500, 6), (260, False, True, None, "relu", 0.0, (), None, 2500, 6),
             (6, True, True, "tensor", "relu", 0.5, (70,), None, 2500, 6), (520, True, False, 1.0, "relu", 0.2, (), None, 2500, 3),
             (12, True, True, "tensor", "relu", 0.5, (), 2, 2500, 6), (64, True, False, 1.0, None, 0.0, (70,), 2, 2500, 6),
             (256, False, True, None, "relu", 0.2, (), 2, 2500, 3), (32, True, True, "tensor", "relu", 0.0, (70,), None, 20000, 3)]


def _hop_id(c):
    return f"d{c[0]}-{'norm' if c[1] else 'plain'}-s{int(c[2])}-self{c[3]}-{c[4]}-p{c[5]}-v{c[7]}-n{c[8]}x{c[9]}"


@pytest.mark.parametrize("case", HOP_CASES, ids=_hop_id)
def test_unignn_hop_vs_float64(case, monkeypatch):
    from allset_amd import Incidence, dense, ops
    from allset_amd.functional import unignn_hop
    d, use_norm, with_s, self_term, act, p, long_rows, variant, n, per_row = case
    V, E, xe, xs, s, G = hop_inputs(d, long_rows, n, per_row)
    inc = Incidence.from_edge_index(torch.stack([V, E]).to(DEV), n_src=n, n_dst=n)
    deg = torch.bincount(V, minlength=n)
    assert bool((deg == 0).any()) and (not long_rows or int(deg.max()) >= max(long_rows))
    built = d % 4 == 0 and d <= 512
    assert ops.unignn_hop_supported(xe.float().to(DEV), xs.float().to(DEV)) == built
    if variant is None and built and d <= 256:               # the library's choice follows the mean degree above 16384 rows
        assert inc.by_src.variant("segreduce", n) == (2 if (n > 16384 and V.numel() < 6 * n) else 1)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    c64 = torch.tensor([1.3], dtype=torch.float64, requires_grad=True)
    dxe, dxs = (t.float().to(DEV).requires_grad_(True) for t in (xe, xs))
    dc = c64.detach().float().to(DEV).requires_grad_(True)
    kw = dict(s=s.float().to(DEV) if with_s else None, use_norm=use_norm, act=act, p=p, variant=variant)
    if self_term is not None:
        kw.update(xs=dxs, c=dc if self_term == "tensor" else self_term)
    y = unignn_hop(dxe, inc, **kw)
    (y * G.float().to(DEV)).sum().backward()
    assert len(seeds) == (1 if p > 0 else 0)
    mask = dense.dropout_scale((n, d), p, seeds[0], DEV).cpu().double() if p > 0 else None
    if mask is not None:
        assert abs(float((mask > 0).double().mean()) - (1 - p)) < 0.02
    lxe, lxs = xe.clone().requires_grad_(True), xs.clone().requires_grad_(True)
    okw = dict(s=s if with_s else None, use_norm=use_norm, act=act, mask=mask)
    if self_term is not None:
        okw.update(xs=lxs, c=c64 if self_term == "tensor" else self_term)
    rep = {}
    yo = orc.hop(lxe, V, E, n, report=rep, **okw)
    (yo * G).sum().backward()
    if act == "relu":                                         # (a priori: the random inputs keep clear of the kink)
        pre = orc.hop(xe, V, E, n, **dict(okw, act=None, mask=None, xs=xs if self_term is not None else None)).detach().abs()
        assert float((pre / pre.amax(dim=1, keepdim=True).clamp_min(1e-300))[pre != 0].min()) > 1e-7
    _close(y, yo, "y")
    _close(dxe.grad, lxe.grad, "gxe")
    if self_term is not None:
        _close(dxs.grad, lxs.grad, "gxs")
    if self_term == "tensor":
        _close(dc.grad, c64.grad, "gc")
    if built:
        y2, t = ops.unignn_hop_fwd(inc.by_src, dxe.detach(), n, kw["s"], dxs.detach() if self_term is not None else None,
                                   dc.detach() if self_term == "tensor" else (self_term or 1.0), use_norm, act, p,
                                   seeds[0] if p > 0 else 0, None, variant)
        assert torch.equal(y2, y.detach())                    # bit-identical from run to run
        if use_norm:
            _close(t, rep["t"], "t")
            if self_term is None:
                assert float(t[(deg == 0).to(DEV)].abs().max()) == 0.0
        else:
            assert t is None
    if use_norm:
        # the scale is a CONSTANT of the backward: differentiating through the norm gives another gxe, further away than the tolerance
        other = xe.clone().requires_grad_(True)
        (orc.hop(other, V, E, n, detach=False, **dict(okw, xs=xs if self_term is not None else None,
                                                       c=float(c64.detach()) if self_term == "tensor" else okw.get("c", 1.0))) * G).sum().backward()
        assert _fails(dxe.grad, other.grad)
    if use_norm and self_term is not None:
        # the self term enters BEFORE the norm: adding it behind the norm is another function, further away than the tolerance
        wrong = orc.hop(xe, V, E, n, self_after_norm=True, **dict(okw, xs=xs, c=float(c64.detach()) if self_term == "tensor" else self_term))
        assert _fails(y, wrong)


def test_hop_cases_cover_the_kernel_paths():
    widths = {c[0] for c in HOP_CASES}
    assert widths >= {4, 12, 64, 128, 256, 512, 6, 520} and any(256 < w < 512 for w in widths)
    assert any(c[7] == 2 for c in HOP_CASES) and any(c[7] is None and c[0] <= 256 and c[8] > 16384 and c[9] < 6 for c in HOP_CASES)
    assert {c[1] for c in HOP_CASES} == {True, False} and {c[3] for c in HOP_CASES} == {None, 1.0, "tensor"}
    assert any(c[5] > 0 and c[0] <= 256 for c in HOP_CASES) and any(c[5] > 0 and c[0] > 256 for c in HOP_CASES)


# (heads, channels, with s, long rows, variant)
EDGE_CASES = [(1, 4, True, (), None), (2, 16, True, (70,), None), (4, 32, False, (70, 1500), None), (8, 32, True, (70,), None),
              (3, 96, True, (70,), None), (1, 512, False, (1100,), None), (5, 64, True, (), None), (8, 64, True, (70,), None),
              (2, 16, True, (70,), 2), (1, 256, False, (), 2), (3, 12, True, (), 2), (1, 7, True, (70,), None), (2, 6, False, (), None),
              (1, 520, True, (), None)]


@pytest.mark.parametrize("case", EDGE_CASES, ids=lambda c: f"H{c[0]}-C{c[1]}-s{int(c[2])}-v{c[4]}")
def test_unigat_edge_vs_float64(case):
    from allset_amd import Incidence, ops
    from allset_amd.functional import unigat_edge
    H, C, with_s, long_rows, variant = case
    d, n = H * C, 2500
    V, E, x, _, s, G = hop_inputs(d, long_rows, n, 6, seed=1)
    g = torch.Generator().manual_seed(5)
    att = torch.randn(1, H, C, generator=g, dtype=torch.float32).double()
    Ga = torch.randn(n, H, generator=g, dtype=torch.float32).double()
    inc = Incidence.from_edge_index(torch.stack([V, E]).to(DEV), n_src=n, n_dst=n)
    assert bool((torch.bincount(E, minlength=n) == 0).any())
    assert ops.unignn_v2e_att_supported(x.float().to(DEV), H) == (C % 4 == 0 and d <= 512)
    dx, da = x.float().to(DEV).requires_grad_(True), att.float().to(DEV).requires_grad_(True)
    xe, ae = unigat_edge(dx, inc, s.float().to(DEV) if with_s else None, da, H, variant=variant)
    ((xe * G.float().to(DEV)).sum() + (ae * Ga.float().to(DEV)).sum()).backward()
    lx, la = x.clone().requires_grad_(True), att.clone().requires_grad_(True)
    xo, ao = orc.edge_logits(lx, V, E, n, s if with_s else None, la, H)
    ((xo * G).sum() + (ao * Ga).sum()).backward()
    _close(xe, xo, "xe")
    _close(ae, ao, "ae")
    _close(dx.grad, lx.grad, "gx")
    _close(da.grad, la.grad, "gatt_e")
    xe2, ae2 = unigat_edge(dx.detach(), inc, s.float().to(DEV) if with_s else None, da.detach(), H, variant=variant)
    assert torch.equal(xe, xe2) and torch.equal(ae, ae2)


# (rows, width, use_norm, skip, act, p)
TAIL_CASES = [(300, 24, True, True, "relu", 0.0), (300, 24, True, False, "relu", 0.5), (1, 4, False, True, None, 0.0),
              (777, 7, True, True, None, 0.2), (513, 130, False, False, "relu", 0.5), (64, 512, True, True, "relu", 0.2),
              (1000, 33, False, True, None, 0.5), (2500, 64, True, False, None, 0.0), (129, 6, False, False, None, 0.2)]


@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: f"{c[0]}x{c[1]}-norm{int(c[2])}-skip{int(c[3])}-{c[4]}-p{c[5]}")
def test_row_tail_vs_float64(case, monkeypatch):
    from allset_amd import dense
    from allset_amd.functional import unignn_row_tail
    n, d, use_norm, with_skip, act, p = case
    g = torch.Generator().manual_seed(1000 * n + d)
    a = torch.randn(n, d, generator=g, dtype=torch.float32).double()
    a[n // 2] = 0                                             # a zero row: t = 0
    skip = torch.randn(n, d, generator=g, dtype=torch.float32).double()
    G = torch.randn(n, d, generator=g, dtype=torch.float32).double()
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    da, ds = a.float().to(DEV).requires_grad_(True), skip.float().to(DEV).requires_grad_(True)
    y = unignn_row_tail(da, skip=ds if with_skip else None, use_norm=use_norm, act=act, p=p)
    (y * G.float().to(DEV)).sum().backward()
    assert len(seeds) == (1 if p > 0 else 0)
    la, ls = a.clone().requires_grad_(True), skip.clone().requires_grad_(True)
    z = orc.row_norm(la) if use_norm else la
    z = z + ls if with_skip else z                            # the norm first, the skip term behind it
    yo = torch.relu(z) if act == "relu" else z
    if p > 0:
        mask = dense.dropout_scale((n, d), p, seeds[0], DEV).cpu().double()
        assert set(mask.unique().tolist()) <= {0.0, float(torch.tensor(1.0 / (1.0 - p), dtype=torch.float32))}
        yo = yo * mask
    (yo * G).sum().backward()
    _close(y, yo, "y")
    _close(da.grad, la.grad, "ga")
    if with_skip:
        _close(ds.grad, ls.grad, "gskip")
    if use_norm and with_skip and n > 1:
        wrong = orc.row_norm(a + skip)                        # the other order (skip in front of the norm) is another function
        assert _fails(y, (torch.relu(wrong) if act == "relu" else wrong) * (mask if p > 0 else 1.0))


def test_unigat_edge_takes_a_misaligned_att_view():
    from allset_amd import Incidence
    from allset_amd.functional import unigat_edge
    H, C, n = 2, 16, 500
    V, E, x, _, s, _ = hop_inputs(H * C, (), n, 6, seed=3)
    inc = Incidence.from_edge_index(torch.stack([V, E]).to(DEV), n_src=n, n_dst=n)
    buf = torch.randn(H * C + 1, device=DEV)
    att = buf[1:]
    assert att.data_ptr() % 16 != 0
    xe, ae = unigat_edge(x.float().to(DEV), inc, None, att, H)
    xe2, ae2 = unigat_edge(x.float().to(DEV), inc, None, att.clone(), H)
    assert torch.equal(xe, xe2) and torch.equal(ae, ae2)


def test_c_entries_validate_their_arguments():
    from allset_amd import _lib
    from allset_amd.functional import unigat_edge, unignn_hop
    lib = _lib.load()
    assert lib.allset_unignn_supported() == 1
    t = torch.zeros(4096, device=DEV)
    i = torch.zeros(8, dtype=torch.int32, device=DEV)
    P, I = t.data_ptr(), i.data_ptr()

    def hop(variant=1, nnz=0, rowptr=I, xe=P, xs=P, y=P, t_out=P, ld=8, use_norm=1, act=1, p=0.0, d=8, n_t=2, n_s=2):
        return lib.allset_unignn_hop_fwd(variant, nnz, 0, rowptr, I, P, xe, ld, xs, ld, 1.0, 0, use_norm, act, p, 0, 0, y, ld, t_out, n_t,
                                         n_s, d, 0)

    def edge(variant=1, nnz=0, rowptr=I, x=P, xe=P, ae=P, att=P, ld=8, H=2, C=4, n_t=2, n_s=2):
        return lib.allset_unignn_v2e_att_fwd(variant, nnz, 0, rowptr, I, P, x, ld, att, xe, ld, ae, n_t, n_s, H, C, 0)

    err = lib.allset_last_error
    assert hop() == 0 and err() == b"" and hop(variant=2) == 0 and hop(variant=0) == 0 and hop(xs=0) == 0
    assert edge() == 0 and err() == b"" and edge(variant=2) == 0
    torch.cuda.synchronize()
    assert hop(rowptr=0) == -1 and b"null" in err()
    assert hop(y=0) == -1 and b"null" in err()
    assert hop(t_out=0) == -1 and b"t_out" in err()
    assert hop(t_out=0, use_norm=0) == 0
    assert hop(nnz=1, xe=0) == -1 and b"null" in err()
    assert hop(n_t=-1) == -1 and b"negative" in err()
    assert hop(ld=4) == -1 and b"leading dimension" in err()
    assert hop(variant=3) == -1 and b"variant" in err()
    assert hop(act=2) == -1 and b"act" in err()
    assert hop(p=1.0) == -1 and b"dropout" in err()
    assert hop(d=6) == -3 and b"not built" in err()
    assert hop(d=520, ld=520) == -3 and b"not built" in err()
    assert hop(d=320, ld=320, variant=2) == -3 and b"short-row" in err()
    assert hop(ld=10) == -3 and b"aligned" in err()
    assert hop(xs=P + 4) == -3 and b"aligned" in err()
    assert hop(n_t=0, rowptr=0) == 0 and err() == b""
    assert edge(C=3, ld=8) == -3 and b"not built" in err()
    assert edge(H=2, C=260, ld=520) == -3 and b"not built" in err()
    assert edge(ae=0) == -1 and b"null" in err()
    assert edge(ld=4) == -1 and b"leading dimension" in err()
    assert edge(x=P + 4) == -3 and b"aligned" in err()
    assert edge(H=5, C=64, ld=320, variant=2) == -3 and b"short-row" in err()
    torch.cuda.synchronize()
    with pytest.raises(_lib.AllSetHipError):
        unignn_hop(torch.zeros(2, 8), None)                                       # CPU tensors
    with pytest.raises(_lib.AllSetHipError):
        unigat_edge(torch.zeros(2, 8), None, None, torch.zeros(8), 2)


# ---- model level -----------------------------------------------------------------------------------------------------------------
def _product(name, train=False):
    import test_unignn_reference as ref
    c = gc.spec(name)
    fx = gc.load(ref.FILE_OF[name])
    model, args, pairs = ref.product_model(c, fx, name)
    model.load_state_dict({k: v.float() for k, v in gc.perturb(model.state_dict(), c).items()})
    model = model.to(DEV).train(train)
    args.degV, args.degE = args.degV.to(DEV), args.degE.to(DEV)
    x = torch.from_numpy(gc.raw_data(c)[0])
    return c, fx, model, pairs, x


def _eval_cases():
    return [n for n in sorted(gc.CASES) if not gc.spec(n)["train"]]


@pytest.mark.parametrize("arith", ["auto", "bf16x6"])
@pytest.mark.parametrize("name", _eval_cases())
def test_model_equals_recorded_reference(name, arith):
    from allset_amd import dense
    c, fx, model, pairs, x = _product(name)
    dx = x.float().to(DEV).requires_grad_(True)
    with dense.arithmetic(arith):
        out = model(dx, pairs[0], pairs[1]) if c["kind"] == "conv" else model(dx)
        G = torch.from_numpy(gc.cotangent(c, out.shape[0]))
        (out * G.float().to(DEV)).sum().backward()

    def scale(k):
        kind, v = gc.result(fx, name, k)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    gc.assert_result(out, fx, name, "out", rtol=1e-4, atol=1e-4 * scale("out"))
    gc.assert_result(dx.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"))
    nograd = {str(s) for s in fx[f"{name}/nograd"]}
    for k, p in model.named_parameters():
        if k in nograd:
            assert p.grad is None, k                                               # att_v: unused, as in the reference
        else:
            gc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"))


@pytest.mark.parametrize("arith", ["auto", "bf16x6"])
@pytest.mark.parametrize("name", [n for n in sorted(gc.CASES) if gc.spec(n)["train"]] + ["gcn2_L2_h2_norm", "gat_L2_h2_norm_c5"])
def test_training_mode_model_with_product_masks(monkeypatch, name, arith):
    import test_unignn_reference as ref
    from allset_amd import dense
    c, fx, model, pairs, x = _product(name, train=True)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    dx = x.float().to(DEV).requires_grad_(True)
    with dense.arithmetic(arith):
        out = model(dx)
        G = torch.from_numpy(gc.cotangent(c, out.shape[0]))
        (out * G.float().to(DEV)).sum().backward()
    assert len(seeds) == c["L"]
    shapes, ps = [(c["n_v"], c["F"])] + [(c["n_v"], c["d"])] * (c["L"] - 1), [gc.INPUT_DROP] + [gc.DROPOUT] * (c["L"] - 1)
    masks = [dense.dropout_scale(s, p, sd_, DEV).cpu().double() for s, p, sd_ in zip(shapes, ps, seeds)]
    sd64 = {k: v.detach().cpu().double() for k, v in model.state_dict().items()}
    lo, xo, sd, margins = ref.oracle_run(c, fx, name, sd64=sd64, masks=masks)
    print("margins:", ["%.3e" % m for m in margins])
    assert min(margins, default=1.0) > gc.RELU_MARGIN
    _close(out, lo, "out")
    _close(dx.grad, xo.grad, "grad_x")
    for k, p in model.named_parameters():
        if k.endswith("att_v"):
            assert p.grad is None
        else:
            _close(p.grad, sd[k].grad, f"grad:{k}")


def test_gin_eps_is_followed_by_a_replayed_graph():
    c, fx, model, pairs, x = _product("gin_L2_h2")
    dx = x.float().to(DEV)
    with torch.no_grad():
        eager0 = model(dx).clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            for _ in range(2):
                model(dx)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = model(dx)
        graph.replay()
        torch.cuda.synchronize()
        torch.testing.assert_close(out, eager0, rtol=0, atol=0)
        for conv in list(model.convs) + [model.conv_out]:
            conv.eps.add_(0.75)
        graph.replay()
        torch.cuda.synchronize()
        eager1 = model(dx)
        torch.testing.assert_close(out, eager1, rtol=0, atol=0)
        assert float((eager1 - eager0).abs().max()) > 1e-3


@pytest.mark.parametrize("name", ["gcn_L2_h2_sum_norm", "gcn2_L2_h2_norm", "gin_L2_h2", "sage_L2_h1_mean2", "gat_L2_h2_norm_c5"])
def test_graphed_train_step_equals_eager(name):
    from allset_amd import dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    from types import SimpleNamespace
    c, fx, model, pairs, x = _product(name)
    data = SimpleNamespace(x=x.float().to(DEV))
    y = torch.randint(0, c["C"], (x.shape[0],), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1))
    loss_fn = lambda out: torch.nn.functional.nll_loss(out, y)
    eager = copy.deepcopy(model)
    eager._graph = None
    opt_e = FusedAdam(eager.parameters(), lr=0.01, weight_decay=5e-4)
    eager.eval()
    for _ in range(3):
        opt_e.zero_grad()
        with dense.deferred_param_grads():
            loss_fn(eager(data)).backward()
        opt_e.step()
    step = GraphedTrainStep(model, data, loss_fn, FusedAdam(model.parameters(), lr=0.01, weight_decay=5e-4), train_mode=False)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


@pytest.mark.parametrize("method,extra", [("UniGCN", []), ("UniGCN2", ["--UniGNN_use-norm"]), ("UniGIN", ["--heads", "2"]),
                                          ("UniSAGE", ["--UniGNN_second_aggregate", "mean", "--hip_graph", "0"]),
                                          ("UniGAT", ["--heads", "2", "--UniGNN_activation", "prelu"])])
def test_train_driver_runs_and_learns(tmp_path, method, extra):
    cmd = [sys.executable, "-m", "allset_amd.train", "--method", method, "--dname", "synthetic", "--epochs", "50", "--runs", "2",
           "--lr", "0.01", "--res_root", str(tmp_path)] + (extra if "--hip_graph" in extra else extra + ["--hip_graph", "1"])
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout
    train = float(re.search(r"Highest Train: ([0-9.]+) ±", res.stdout).group(1))
    valid = float(re.search(r"Highest Valid: ([0-9.]+) ±", res.stdout).group(1))
    test = float(re.search(r"Final Test: ([0-9.]+) ±", res.stdout).group(1))
    print(method, "highest train / highest valid / final test accuracy", train, valid, test)
    # held-out vertices, five balanced classes (chance 20 %): a model that only memorises its training split stays at chance there.
    # The planted partition fills 80 % of every hyperedge from one class, so a working hop lifts both well past 2.5 x chance.
    assert valid > 50.0 and test > 50.0
