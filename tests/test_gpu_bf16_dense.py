"""GPU: the bf16 kernels of the dense surface are the fp32 arithmetic rounded ONCE.  LayerNorm and residual LayerNorm (csrc/dense.hip
``ln_*_bf16``), the weight gradient (``wgrad_bf16_tr_kernel`` at every width, masked and with the auxiliary rows, and the tiled
kernel) with the reduction that rounds it, and Adam (csrc/optim.hip) are each compared with float64 on the same bf16-rounded inputs
under ``bf16_cases.within_one_rounding`` (half a bf16 ulp on top of the fp32 kernels' own 1e-4); on the exact tables of
tests/bf16_dense_cases.py the stored BITS must be ``float64 -> .float() -> .bfloat16()``.  Adam is held to the bounds derived in
``bf16_dense_cases.adam_within``.  tests/test_bf16_dense_cases_host.py vouches for the cases from float64 alone.  A device result is
never an expected value; a dropout mask read off the forward output, and the state a multi-step run held before a step, are data.
Each test prints ``max |got - ref| / (ulp/2)`` before it asserts."""
import os
import sys
from ctypes import byref, c_int64

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_dense_cases as dc  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
SEED = 20240611
NAN = float("nan")


def _dev(t, device, ld=None):
    """float64 holding bf16 values -> the bf16 device tensor; ``ld`` above the width: a view into a wider buffer whose other
    columns hold NaN."""
    if t is None:
        return None
    tb = t.to(BF16)
    assert torch.equal(tb.double(), t)
    if ld is None or ld == t.shape[1]:
        return tb.to(device)
    buf = torch.full((t.shape[0], ld), NAN, dtype=BF16, device=device)
    buf[:, :t.shape[1]] = tb.to(device)
    view = buf[:, :t.shape[1]]
    assert view.stride(0) == ld
    return view


def _stats(r, device):
    return torch.stack([r["mean"], r["rstd"]], dim=1).float().to(device)


def _keep(y, unsure, p):
    """The dropout factor per element from the stored output: a stored zero away from the unsure band is a dropped element."""
    kept = (y.detach().cpu().float() != 0) | unsure
    return kept, kept.double() / (1.0 - float(np.float32(p)))


def _masked_rule(got, ref, sure, what):
    dc.assert_one_rounding(got.detach().cpu().double()[sure], ref[sure], what)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------------------
def _run_layer_norm(c, device):
    from allset_amd import dense
    t = dc.ln_inputs(c.n, c.d)
    x, G, gamma, beta = t["x"], t["G"], t["gamma"], t["beta"]
    xd, gd, bd = _dev(x, device, c.ld), _dev(gamma[None], device)[0], _dev(beta[None], device)[0]
    y, stats = dense.ln_fwd(xd, gd, bd, dc.LN_EPS, c.relu_in, c.p, SEED)
    assert y.dtype == BF16 and tuple(y.shape) == (c.n, c.d) and stats.dtype == torch.float32
    r0 = dc.ln_reference(x, gamma, beta, None, c.relu_in)
    unsure = dc.unsure_elements(r0["pre"], False, c.p)
    assert float(unsure.double().mean()) <= dc.UNSURE_CAP
    keep = None
    if c.p > 0:
        kept, keep = _keep(y, unsure, c.p)
        if kept.numel() >= 4096:
            assert abs(float(kept.double().mean()) - (1 - c.p)) < 0.05
        assert c.n * c.d < 64 or not bool(kept.all())
        G = torch.where(unsure, torch.zeros_like(G), G)
    r = dc.ln_reference(x, gamma, beta, G, c.relu_in, keep=keep)
    _masked_rule(y, r["y"], ~unsure, f"ln {c.id} y")
    dc.close_fp32(stats[:, 0], r["mean"], f"ln {c.id} mean")
    dc.close_fp32(stats[:, 1], r["rstd"], f"ln {c.id} rstd")
    gx, dg, db = dense.ln_bwd(_dev(G, device, c.ld), xd, _stats(r, device), gd, c.relu_in, c.p, SEED)
    assert gx.dtype == BF16 and dg.dtype == BF16 and db.dtype == BF16
    dc.assert_one_rounding(gx, r["gx"], f"ln {c.id} gx")
    dc.assert_one_rounding(dg, r["dgamma"], f"ln {c.id} dgamma")
    dc.assert_one_rounding(db, r["dbeta"], f"ln {c.id} dbeta")
    if c.relu_in:
        off = x <= 0                                                        # -0.0 and +0.0 included
        assert bool(off.any()) and bool((gx.cpu().float()[off] == 0).all())
    _, dg2, db2 = dense.ln_bwd(_dev(G, device, c.ld), xd, _stats(r, device), gd, c.relu_in, c.p, SEED, want_gx=False)
    assert torch.equal(dg2.view(torch.int16), dg.view(torch.int16)) and torch.equal(db2.view(torch.int16), db.view(torch.int16))


@pytest.mark.parametrize("c", dc.LN_CASES + dc.LN_LD_CASES, ids=lambda c: c.id)
def test_layer_norm_is_one_rounding_from_float64(c, device):
    _run_layer_norm(c, device)


def _partials_cap(d):
    from allset_amd import _lib
    npart = c_int64(0)
    _lib.check(_lib.load().allset_ln_bwd_bf16_partials(10 ** 7, d, byref(npart)), "allset_ln_bwd_bf16_partials")
    return npart.value


def test_layer_norm_backward_walks_two_rows_per_lane_group(device):
    """One row more than the capped backward grid covers in one sweep (the cap is read from the ``_partials`` entry): the first
    lane group of the first workgroup walks rows 0 and n - 1.  Plain and residual backward."""
    from allset_amd import dense, _lib
    d = dc.LN_GRID_STRIDE_D
    cap = _partials_cap(d)
    n = dc.ln_grid_stride_rows(cap)
    npart = c_int64(0)
    _lib.check(_lib.load().allset_ln_bwd_bf16_partials(n, d, byref(npart)), "allset_ln_bwd_bf16_partials")
    assert npart.value == cap == dc.ln_bwd_partials(n, d) and cap * dc.ln_groups(d) == n - 1
    t = dc.ln_inputs(n, d, "stride")
    x, G, gamma, beta, colb, res = (t[k] for k in ("x", "G", "gamma", "beta", "colb", "res"))
    xd, Gd, gd, bd = _dev(x, device), _dev(G, device), _dev(gamma[None], device)[0], _dev(beta[None], device)[0]
    r = dc.ln_reference(x, gamma, beta, G, True)
    gx, dg, db = dense.ln_bwd(Gd, xd, _stats(r, device), gd, True, 0.0, SEED)
    dc.assert_one_rounding(gx, r["gx"], "ln grid-stride gx")
    dc.assert_one_rounding(dg, r["dgamma"], "ln grid-stride dgamma")
    dc.assert_one_rounding(db, r["dbeta"], "ln grid-stride dbeta")
    r = dc.ln_reference(x, gamma, beta, G, colb=colb, res=res)
    gs, dg, db, dcb = dense.ln_res_bwd(Gd, xd, _dev(colb[None], device)[0], _dev(res, device), _stats(r, device), gd, bd, False, 0.0, SEED)
    dc.assert_one_rounding(gs, r["gx"], "ln-res grid-stride gs")
    dc.assert_one_rounding(dg, r["dgamma"], "ln-res grid-stride dgamma")
    dc.assert_one_rounding(db, r["dbeta"], "ln-res grid-stride dbeta")
    dc.assert_one_rounding(dcb, r["dcolb"], "ln-res grid-stride dcolb")


def test_layer_norm_backward_refuses_a_gradient_it_would_have_to_round(device):
    """An fp32 ``gy`` next to bf16 activations: a cast inside the wrapper would round the gradient before the kernel rounds the
    result -- two roundings.  Refused, as ``ln_res_bwd`` refuses it."""
    from allset_amd import dense, _lib
    t = dc.ln_inputs(5, 64)
    r = dc.ln_reference(t["x"], t["gamma"], t["beta"])
    with pytest.raises(_lib.AllSetHipError, match="bfloat16"):
        dense.ln_bwd(t["G"].float().to(device), _dev(t["x"], device), _stats(r, device), _dev(t["gamma"][None], device)[0], False, 0.0, SEED)


# ---- residual LayerNorm ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", dc.LN_RES_CASES, ids=lambda c: c.id)
def test_layer_norm_res_is_one_rounding_from_float64(c, device):
    from allset_amd import dense
    t = dc.ln_inputs(c.n, c.d)
    x, G, gamma, beta = t["x"], t["G"], t["gamma"], t["beta"]
    colb, res = (t["colb"] if c.has_colb else None), (t["res"] if c.has_res else None)
    xd, gd, bd = _dev(x, device), _dev(gamma[None], device)[0], _dev(beta[None], device)[0]
    cd, rd = (_dev(colb[None], device)[0] if c.has_colb else None), _dev(res, device)
    y, stats = dense.ln_res_fwd(xd, cd, rd, gd, bd, dc.LN_EPS, c.relu_out, c.p, SEED)
    assert y.dtype == BF16 and tuple(y.shape) == (c.n, c.d)
    r0 = dc.ln_reference(x, gamma, beta, None, False, colb, res)
    unsure = dc.unsure_elements(r0["pre"], c.relu_out, c.p)
    assert float(unsure.double().mean()) <= dc.UNSURE_CAP
    keep = None
    if c.p > 0:
        kept, keep = _keep(y, unsure, c.p)
        live = (r0["pre"] > dc.UNSURE) if c.relu_out else torch.ones_like(kept)
        assert abs(float(kept[live].double().mean()) - (1 - c.p)) < (0.05 if int(live.sum()) >= 4096 else 0.2)
    G = torch.where(unsure, torch.zeros_like(G), G)
    r = dc.ln_reference(x, gamma, beta, G, False, colb, res, c.relu_out, keep)
    what = f"ln-res {c.id}"
    _masked_rule(y, r["y"], ~unsure, what + " y")
    dc.close_fp32(stats[:, 0], r["mean"], what + " mean")
    dc.close_fp32(stats[:, 1], r["rstd"], what + " rstd")
    gs, dg, db, dcb = dense.ln_res_bwd(_dev(G, device), xd, cd, rd, _stats(r, device), gd, bd, c.relu_out, c.p, SEED)
    assert all(v.dtype == BF16 for v in (gs, dg, db, dcb))
    dc.assert_one_rounding(gs, r["gx"], what + " gs")
    if c.has_res:
        dc.assert_one_rounding(gs, r["gres"], what + " res gradient")
    dc.assert_one_rounding(dg, r["dgamma"], what + " dgamma")
    dc.assert_one_rounding(db, r["dbeta"], what + " dbeta")
    dc.assert_one_rounding(dcb, r["dcolb"] if c.has_colb else r["gx"].sum(0), what + " dcolb")


@pytest.mark.parametrize("d,heads", dc.LN_PMA_SHAPES)
def test_layer_norm_res_backward_with_the_pooling_statistics(d, heads, device):
    """``ln_res_bwd_pma``: the residual backward plus, per (row, head), ``m + log(l + 1e-16)`` (FLT_MAX exactly where l = 0) and
    ``<x, gs>`` on the stored bf16 ``gs`` -- which is itself held to the one-rounding rule here."""
    from allset_amd import dense
    assert dense.ln_res_bwd_pma_supported(d, heads, BF16)
    n = dc.LN_PMA_ROWS
    t = dc.ln_inputs(n, d, "pma")
    x, G, gamma, beta, colb = (t[k] for k in ("x", "G", "gamma", "beta", "colb"))
    m, l, empty = dc.pma_ml(n, heads)
    r = dc.ln_reference(x, gamma, beta, G, colb=colb)
    gs, dg, db, dcb, pst = dense.ln_res_bwd_pma(_dev(G, device), _dev(x, device), _dev(colb[None], device)[0], _stats(r, device),
                                                _dev(gamma[None], device)[0], _dev(beta[None], device)[0], m.float().to(device), l.float().to(device))
    what = f"ln-res-pma d{d} H{heads}"
    assert gs.dtype == BF16 and pst.dtype == torch.float32 and tuple(pst.shape) == (n, heads, 2)
    dc.assert_one_rounding(gs, r["gx"], what + " gs")
    dc.assert_one_rounding(dg, r["dgamma"], what + " dgamma")
    dc.assert_one_rounding(db, r["dbeta"], what + " dbeta")
    dc.assert_one_rounding(dcb, r["dcolb"], what + " dcolb")
    want = dc.pma_stats_dense_reference(x, gs.cpu().double(), m, l, heads)
    got = pst.cpu()
    assert bool(empty.any()) and bool((got[empty][..., 0] == dc.FLT_MAX).all())
    dc.close_fp32(got[~empty][..., 0], want[~empty][..., 0], what + " stats M")
    dc.close_fp32(got[..., 1], want[..., 1], what + " stats <x, gs>")


# ---- weight gradient ---------------------------------------------------------------------------------------------------------------------
def _check(got, ref, kind, what):
    assert got.dtype == BF16 and tuple(got.shape) == tuple(ref.shape), what
    if kind == "general":
        dc.assert_one_rounding(got, ref, what)
        return
    want = ref.float().to(BF16)
    same = dc.bits_equal(got, want)
    print(f"{what}: {int((~same).sum())} of {same.numel()} elements differ from the expected bits")
    if not bool(same.all()):
        i = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{what}: {int((~same).sum())} of {same.numel()} elements are not the expected bf16 bits; first at {i}: got "
                             f"{float(got[i])!r}, float64 {float(ref[i])!r}, expected {float(want[i])!r}")


@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("c", dc.WG_FULL_CASES + dc.WG_TILED_CASES, ids=lambda c: c.id)
def test_weight_gradient_is_one_rounding_from_float64(c, kind, device):
    from allset_amd import dense, _lib
    ns = c_int64(0)
    _lib.check(_lib.load().allset_wgrad_bf16_slices(c.n, c.O, c.I, byref(ns)), "allset_wgrad_bf16_slices")
    assert ns.value == dc.wgrad_bf16_slices(c.n, c.O, c.I)
    ga, u, _ = dc.wgrad_tables(c.n, c.O, c.I, kind)
    gad, ud = _dev(ga, device, c.ld_a), _dev(u, device, c.ld_u)
    ref_w, ref_b = dc.wgrad_reference(ga, u)
    gw, gb = dense.wgrad(gad, ud)
    _check(gw, ref_w, kind, f"wgrad {c.id} {kind} gW")
    _check(gb, ref_b, kind, f"wgrad {c.id} {kind} gb")
    gw2, none = dense.wgrad(gad, ud, want_bias=False)
    assert none is None and torch.equal(gw2.view(torch.int16), gw.view(torch.int16))


@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("c", dc.WG_EX2_CASES, ids=lambda c: c.id)
def test_masked_weight_gradient_and_auxiliary_rows_are_one_rounding_from_float64(c, kind, device):
    """``wgrad_bf16_ex2``: the relu bit mask of a real ``linear_bf16_fwd_mask`` applied to ``ga`` on the way (the reference masks by
    ``y > 0`` of that forward's stored output), and the four auxiliary rows from ``g4`` rounded to bf16."""
    from allset_amd import dense
    assert dense.wgrad_bf16_ex2_supported(c.O, c.I, c.bits, c.aux)
    ga, u, g4 = dc.wgrad_tables(c.n, c.O, c.I, kind)
    gad, ud = _dev(ga, device), _dev(u, device)
    bits = mask = None
    if c.bits:
        Wf = _dev(dc.bf16_round(dc.general_table(c.O, c.I, "wf") / 16), device)
        bf = _dev(dc.general_table(1, c.O, "bf"), device)[0]
        y, bits = dense.linear_bf16_fwd_mask(ud, Wf, bf)
        mask = (y.float() > 0).cpu()
        assert 0.2 < float(mask.double().mean()) < 0.8
    refs = dc.wgrad_reference(ga, u, mask, g4 if c.aux else None)
    got = dense.wgrad_bf16_ex2(gad, ud, bits=bits, g4=g4.float().to(device) if c.aux else None)
    assert len(got) == len(refs)
    for g, r, name in zip(got, refs, ("gW", "gb", "gWa", "gba")):
        _check(g, r, kind, f"wgrad_ex2 {c.id} {kind} {name}")


@pytest.mark.parametrize("kind", ["exact", "general"])
@pytest.mark.parametrize("P,M,stride", dc.REDUCE_CASES)
def test_reduce_partials_to_bf16_is_one_rounding_from_float64(P, M, stride, kind, device):
    from allset_amd import dense, _lib
    assert bool(_lib.load().allset_reduce_partials_is_tree(P, M)) == dc.reduce_is_tree(P, M)
    part = dc.reduce_partials_table(P, stride, kind)
    pd = part.float().to(device)
    if stride > M:
        pd[:, M:] = NAN                                                    # (columns behind M are not read)
    got = dense.reduce_partials_to(pd, M, BF16)
    _check(got, part[:, :M].sum(0), kind, f"reduce P{P} M{M} stride{stride} {kind}")


# ---- Adam --------------------------------------------------------------------------------------------------------------------------------
def _adam_setup(sizes, bf16, pre, wd, device, what, hyper=None):
    from allset_amd.optim import FusedAdam
    dt = BF16 if bf16 else torch.float32
    host, params = [], []
    for k, n in enumerate(sizes):
        p, g, m, v = dc.adam_state(n, bf16, f"{what}-{k}")
        host.append((p, g, m, v))
        P = torch.nn.Parameter(p.to(dt).to(device))
        P.grad = g.to(dt).to(device)
        params.append(P)
    idle = torch.nn.Parameter(dc.adam_state(5, bf16, "idle")[0].to(dt).to(device))       # no gradient: not touched, no state
    opt = FusedAdam(params + [idle], weight_decay=wd, **(hyper or dc.ADAM_HYPER))
    for P, (p, g, m, v) in zip(params, host):
        opt.state[P] = dict(step=torch.tensor(float(pre), dtype=torch.float32, device=device), exp_avg=m.to(dt).to(device),
                            exp_avg_sq=v.to(dt).to(device))
    return opt, params, idle, host


def _adam_check(opt, P, ref, bf16, what):
    st = opt.state[P]
    dc.assert_adam(st["exp_avg"], ref, "m", bf16, what)
    dc.assert_adam(st["exp_avg_sq"], ref, "v", bf16, what)
    dc.assert_adam(P.detach(), ref, "p", bf16, what)


@pytest.mark.parametrize("wd", dc.ADAM_WD)
@pytest.mark.parametrize("pre", dc.ADAM_PRE_STEPS)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_fused_adam_single_step_from_a_prepared_state(bf16, pre, wd, device):
    """One step from a prepared state against the float64 restatement of csrc/optim.hip's header on the float32-rounded
    hyper-parameters: sizes on both sides of the 2048-element chunk, a zero-element parameter between two others, one live parameter
    more than a pointer table holds (read from ``allset_adam_max_tensors``) and one parameter without a gradient."""
    from allset_amd import _lib
    cap = int(_lib.load().allset_adam_max_tensors())
    sizes = dc.adam_sizes(cap)
    assert len(sizes) == cap + 1 and 0 in sizes
    opt, params, idle, host = _adam_setup(sizes, bf16, pre, wd, device, "single")
    idle_before = idle.detach().clone()
    opt.step()
    for k, (P, (p, g, m, v)) in enumerate(zip(params, host)):
        assert float(opt.state[P]["step"]) == pre + 1
        ref = dc.adam_reference(p, g, m, v, pre + 1, wd=wd, **dc.ADAM_HYPER)
        _adam_check(opt, P, ref, bf16, f"adam {'bf16' if bf16 else 'fp32'} t{pre + 1} wd{wd} tensor {k} ({sizes[k]})")
    assert torch.equal(idle.detach(), idle_before) and len(opt.state[idle]) == 0


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_fused_adam_four_steps_each_from_the_state_the_device_held(bf16, device):
    """The reference of step k starts from the parameters and moments the device held before step k (data, not an expected value)."""
    sizes = [2049, 1, 300]
    opt, params, _, _ = _adam_setup(sizes, bf16, 0, 0.01, device, "multi")
    dt = BF16 if bf16 else torch.float32
    wd32 = float(np.float32(0.01))
    for k in range(4):
        before = []
        for j, P in enumerate(params):
            st = opt.state[P]
            p = P.detach().cpu().double().clone()
            g = dc.adam_state(sizes[j], bf16, f"multi-grad-{k}-{j}")[1]
            g = torch.where((g + wd32 * p).abs() < 0.5 * (wd32 * p).abs(), -g, g)      # (the parameter has moved: adam_state's budget for wd * p, kept)
            P.grad = g.to(dt).to(device)
            before.append((p, g, st["exp_avg"].detach().cpu().double().clone(), st["exp_avg_sq"].detach().cpu().double().clone()))
        opt.step()
        for j, P in enumerate(params):
            assert float(opt.state[P]["step"]) == k + 1
            p, g, m, v = before[j]
            ref = dc.adam_reference(p, g, m, v, k + 1, wd=0.01, **dc.ADAM_HYPER)
            _adam_check(opt, P, ref, bf16, f"adam {'bf16' if bf16 else 'fp32'} step {k + 1} tensor {j}")


def test_fused_adam_bf16_with_zero_learning_rate_leaves_the_parameter_bits(device):
    """lr = 0, wd = 0: every parameter keeps its bits (a +0.0 among them) while the moments still move.  (A parameter of -0.0 is
    not among the inputs: ``p - 0 * x`` is an IEEE subtraction and gives +0.0 where ``x < 0`` -- measured so on the device -- as
    torch.optim.Adam's ``addcdiv_`` does; the value is unchanged.)"""
    hyper = dict(dc.ADAM_HYPER, lr=0.0)
    sizes = [2049, 7]
    opt, params, _, host = _adam_setup(sizes, True, 1, 0.0, device, "frozen", hyper)
    with torch.no_grad():
        params[0][0] = 0.0
    before = [P.detach().clone() for P in params]
    opt.step()
    for P, b, (p, g, m, v) in zip(params, before, host):
        assert torch.equal(P.detach().view(torch.int16), b.view(torch.int16))
        ref = dc.adam_reference(p, g, m, v, 2, wd=0.0, **hyper)
        dc.assert_adam(opt.state[P]["exp_avg"], ref, "m", True, "adam lr 0")
        dc.assert_adam(opt.state[P]["exp_avg_sq"], ref, "v", True, "adam lr 0")
