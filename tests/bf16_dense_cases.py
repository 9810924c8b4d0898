"""The bf16 regime of the dense surface (csrc/dense.hip: LayerNorm, residual LayerNorm, the weight gradient and the partial-sum
reduction; csrc/optim.hip: Adam): the case lists that reach every bf16 instantiation the launchers can select, the input tables,
their float64 references and the acceptance rules.  Imports on the CPU; shared by tests/test_bf16_dense_cases_host.py (which vouches
for every case from float64 alone) and tests/test_gpu_bf16_dense.py (which runs the same lists through the HIP kernels).

The rounding rule, the exact-bits comparison and the fp32 rule are those of tests/bf16_cases.py, imported and not restated: a bf16
kernel runs the fp32 arithmetic and rounds ONCE, at the store.  Every reference is float64 torch / numpy on the bf16- (activations,
parameters, cotangents) or fp32- (statistics, partials, logits' gradients) rounded inputs."""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_structures as hs  # noqa: E402
from bf16_cases import (bf16_round, ulp_bf16, within_one_rounding, assert_one_rounding, bits_equal, close_fp32,  # noqa: E402,F401
                        general_table)

D64 = torch.float64
FLT_MAX = float(np.finfo(np.float32).max)


def _rng(*parts):
    return np.random.default_rng(hs.hash_id("dense-" + "-".join(str(p) for p in parts)))


def f32_round(t):
    return t.float().double()


# ---- LayerNorm: geometry (csrc/dense.hip restated) -------------------------------------------------------------------------------------
WAVES_PER_BLOCK, WAVE, LN_ROWS_PER_GROUP = 4, 64, 4      # common.h kWavesPerBlock / kWave, dense.hip kLnRowsPerGroup
LN_BWD_PARTIALS_CAP = 2048                               # allset_ln_bwd_bf16_partials (the GPU file reads the entry and compares)
LN_EPS = float(np.float32(1e-5))                         # the kernel receives eps as a float
LN_WIDTHS = (8, 40, 64, 72, 128, 200, 256, 264, 504, 512)
LN_LPRS = (8, 16, 32, 64)
UNSURE = 1e-3                                            # |float64 pre-activation| below which a relu / dropout zero is no mask evidence
UNSURE_CAP = 0.005


def ln_bf16_lpr(d):
    """``ln_bf16_lpr``: lanes per row, one lane = 8 columns."""
    assert d % 8 == 0 and 8 <= d <= 512
    return 8 if d <= 64 else (16 if d <= 128 else (32 if d <= 256 else 64))


def ln_groups(d):
    """Lane groups (rows in flight) per workgroup."""
    return WAVES_PER_BLOCK * (WAVE // ln_bf16_lpr(d))


def ln_rows_per_block(d):
    """Rows a forward workgroup owns: the last workgroup clamps its loads to row n - 1."""
    return ln_groups(d) * LN_ROWS_PER_GROUP


def ln_bwd_partials(n, d):
    """``allset_ln_bwd_bf16_partials``: the backward grid (one partial row per workgroup)."""
    g = ln_groups(d)
    return max(1, min(LN_BWD_PARTIALS_CAP, -(-n // g)))


def ln_rows(d):
    """One row, a few, more than one wave's worth, and one row more than a forward workgroup owns."""
    return (1, 5, 37, ln_rows_per_block(d) + 1)


LnCase = namedtuple("LnCase", "id n d ld relu_in p")
LN_OPTIONS = [(False, 0.0), (True, 0.0), (False, 0.3), (True, 0.3)]


def _ln_id(n, d, ld, relu_in, p):
    return f"n{n}-d{d}" + (f"-ld{ld}" if ld != d else "") + ("-relu" if relu_in else "") + (f"-p{p}" if p else "")


LN_CASES = [LnCase(_ln_id(n, d, d, r, p), n, d, d, r, p) for d in LN_WIDTHS for n in ln_rows(d) for r, p in LN_OPTIONS]
# rows taken as columns of a wider buffer (ld a multiple of 8; the other columns hold NaN)
LN_LD_CASES = [LnCase(_ln_id(37, 200, 264, r, p), 37, 200, 264, r, p) for r, p in ((False, 0.0), (True, 0.3))]
LN_GRID_STRIDE_D = 512


def ln_grid_stride_rows(partials_cap):
    """One row more than the capped backward grid covers in one sweep: a lane group walks two rows."""
    return partials_cap * ln_groups(LN_GRID_STRIDE_D) + 1


LnResCase = namedtuple("LnResCase", "id n d has_res has_colb relu_out p")


def ln_res_rows(d):
    return (37, ln_rows_per_block(d) + 1)


LN_RES_CASES = [LnResCase(f"n{n}-d{d}-{'res' if r else 'nores'}-{'colb' if c else 'nocolb'}" + ("-relu" if ro else "") + (f"-p{p}" if p else ""),
                          n, d, r, c, ro, p)
                for d in LN_WIDTHS for n in ln_res_rows(d) for r in (False, True) for c in (False, True) for ro in (False, True)
                for p in (0.0, 0.3)]
LN_PMA_SHAPES = [(64, 8), (40, 5), (192, 3), (256, 4), (512, 1), (128, 4)]   # (d, heads); (128, 4): the one LPR (16) the others leave out
LN_PMA_ROWS = 37


def ln_res_instantiations(cases=None, pma=None):
    """The (LPR, HAS_RES, DROP, PMA) the launchers reach for these cases (``ln_res_fwd_bf16`` ignores PMA)."""
    cases = LN_RES_CASES if cases is None else cases
    pma = LN_PMA_SHAPES if pma is None else pma
    return {(ln_bf16_lpr(c.d), c.has_res, c.p > 0, False) for c in cases} | {(ln_bf16_lpr(d), False, False, True) for d, _ in pma}


def ln_res_all_instantiations():
    """What ``allset_ln_res_bwd_bf16`` / ``allset_ln_res_bwd_pma_bf16`` can select: the PMA entry passes no residual and p = 0."""
    return {(l, r, dr, False) for l in LN_LPRS for r in (False, True) for dr in (False, True)} | {(l, False, False, True) for l in LN_LPRS}


def pma_lanes_per_head(d, heads):
    assert d % heads == 0 and (d // heads) % 8 == 0
    g = (d // heads) // 8
    assert g & (g - 1) == 0
    return g


# ---- LayerNorm: tables -----------------------------------------------------------------------------------------------------------------
def ln_inputs(n, d, what="ln"):
    """x, G [n, d], gamma = 1 + 0.2 randn, beta = 0.3 randn, colb = 0.5 randn, res [n, d]: float64 holding bf16 values.  ``x`` carries
    some +0.0 and -0.0 (the first two columns of row 0 and one element in sixteen of the last row)."""
    r = _rng(what, n, d)
    x = bf16_round(torch.from_numpy(r.standard_normal((n, d))))
    G = bf16_round(torch.from_numpy(r.standard_normal((n, d))))
    gamma = bf16_round(torch.from_numpy(1 + 0.2 * r.standard_normal(d)))
    beta = bf16_round(torch.from_numpy(0.3 * r.standard_normal(d)))
    colb = bf16_round(torch.from_numpy(0.5 * r.standard_normal(d)))
    res = bf16_round(torch.from_numpy(r.standard_normal((n, d))))
    x[0, 0], x[0, 1] = 0.0, -0.0
    z = torch.from_numpy(r.integers(0, 16, size=d) == 0)
    x[n - 1] = torch.where(z, torch.from_numpy(np.where(r.integers(0, 2, size=d) == 0, 0.0, -0.0)), x[n - 1])
    return dict(x=x, G=G, gamma=gamma, beta=beta, colb=colb, res=res)


def pma_ml(n, heads):
    """The pooling's fp32 statistics: m = randn, l in [1, 50), and l = m = 0 on rows 0, 3 and n - 1 (targets without incidence)."""
    r = _rng("pma-ml", n, heads)
    m = torch.from_numpy(r.standard_normal((n, heads)).astype(np.float32)).double()
    l = torch.from_numpy((1 + 49 * r.random((n, heads))).astype(np.float32)).double()
    empty = torch.zeros(n, dtype=torch.bool)
    empty[[0, 3, n - 1]] = True
    m[empty], l[empty] = 0.0, 0.0
    return m, l, empty


# ---- LayerNorm: the float64 reference --------------------------------------------------------------------------------------------------
def ln_reference(x, gamma, beta, G=None, relu_in=False, colb=None, res=None, relu_out=False, keep=None):
    """``y = keep * relu_out(LN(relu_in(x + colb + res)))`` in float64 and, with a cotangent ``G``, its gradients by autograd.
    ``keep``: the dropout factor per element (0 or 1 / (1 - p)), data.  Returns pre (the LayerNorm output before relu_out / dropout), y,
    mean, rstd [n] and gx (= the gradient of x and of res), dgamma, dbeta, dcolb."""
    d = x.shape[1]
    leaves = {k: (None if v is None else v.clone().requires_grad_(G is not None)) for k, v in
              dict(x=x, gamma=gamma, beta=beta, colb=colb, res=res).items()}
    s = leaves["x"]
    if colb is not None:
        s = s + leaves["colb"]
    if res is not None:
        s = s + leaves["res"]
    t = F.relu(s) if relu_in else s
    pre = F.layer_norm(t, (d,), leaves["gamma"], leaves["beta"], LN_EPS)
    y = F.relu(pre) if relu_out else pre
    if keep is not None:
        y = y * keep
    td = t.detach()
    mean = td.mean(1)
    out = dict(pre=pre.detach(), y=y.detach(), mean=mean, rstd=1.0 / torch.sqrt(((td - mean[:, None]) ** 2).mean(1) + LN_EPS))
    if G is not None:
        (y * G).sum().backward()
        out.update(gx=leaves["x"].grad, dgamma=leaves["gamma"].grad, dbeta=leaves["beta"].grad,
                   dcolb=None if colb is None else leaves["colb"].grad, gres=None if res is None else leaves["res"].grad)
    return out


def unsure_elements(pre, relu_out, p):
    """bool per element: a zero of the output is no evidence of the relu / dropout mask there."""
    if not relu_out and p == 0.0:
        return torch.zeros_like(pre, dtype=torch.bool)
    return pre.abs() <= UNSURE


def pma_stats_dense_reference(x, gs_stored, m, l, heads):
    """``pma_stats`` [n, H, 2] of ``ln_res_bwd_pma``: (m + log(l + 1e-16), <x[t, h], gs[t, h]>) on the STORED bf16 ``gs`` (the
    convention of ``bf16_cases.pma_stats_reference``); the first entry is FLT_MAX where l = 0."""
    n = x.shape[0]
    M = torch.where(l > 0, m + torch.log(l + 1e-16), torch.full_like(m, FLT_MAX))
    return torch.stack([M, (x.view(n, heads, -1) * gs_stored.view(n, heads, -1)).sum(-1)], dim=-1)


# ---- weight gradient -------------------------------------------------------------------------------------------------------------------
WG_TILE, WG_ROWS = 128, 32                              # dense.hip kWgTile / kWgRows
WG_FULL_WIDTHS = (64, 128, 256)
WG_ROWS_LIST = (1, 31, 33, 257, 1000)
WgCase = namedtuple("WgCase", "id n O I ld_a ld_u")
WG_FULL_CASES = [WgCase(f"n{n}-O{O}-I{I}", n, O, I, O, I) for O in WG_FULL_WIDTHS for I in WG_FULL_WIDTHS for n in WG_ROWS_LIST]
WG_TILED_CASES = [WgCase(f"n{n}-O{O}-I{I}", n, O, I, O, I) for O, I in ((4, 260), (132, 64), (256, 512), (512, 512)) for n in (33, 257)] + \
                 [WgCase("n257-O64-I64-ld68", 257, 64, 64, 68, 68)]     # full-width sizes, rows not 16-byte aligned: the tiled kernel
WG_BITS_WIDTHS = [(128, 128), (128, 256), (256, 128), (256, 256)]         # allset_wgrad_bf16_ex2_supported(O, I, bits, no aux)
WG_EX2_ROWS = (33, 257, 1000)
Ex2Case = namedtuple("Ex2Case", "id n O I bits aux")
WG_EX2_CASES = [Ex2Case(f"n{n}-O{O}-I{I}-bits", n, O, I, True, False) for O, I in WG_BITS_WIDTHS for n in WG_EX2_ROWS] + \
               [Ex2Case(f"n{n}-O256-I256-{'bits-' if b else ''}g4", n, 256, 256, b, True) for b in (False, True) for n in WG_EX2_ROWS]
WG_CENSUS_ROWS = (257, 1000)


def wgrad_bf16_full_width(O, I):
    return O in WG_FULL_WIDTHS and I in WG_FULL_WIDTHS


def wgrad_slices(n, O, I):
    """``allset_wgrad_slices`` (the tiled kernel's split over rows)."""
    tiles = -(-O // WG_TILE) * -(-I // WG_TILE)
    s = 512 // tiles
    by_rows = (n + 255) // 256
    if min(s, by_rows) * tiles < 128:
        by_rows = (n + 127) // 128
    return max(1, min(s, by_rows))


def wgrad_bf16_slices(n, O, I):
    """``allset_wgrad_bf16_slices``."""
    if not wgrad_bf16_full_width(O, I):
        return wgrad_slices(n, O, I)
    return max(1, min(256 if (O, I) == (256, 256) else 512, (n + 255) // 256))


def wgrad_kernel(c, bits=False, aux=False):
    """``('tr', OTN, ITN, MK, AX)`` or ``('tiled',)``: what ``wgrad_bf16_impl`` launches for 16-byte aligned buffers."""
    if wgrad_bf16_full_width(c.O, c.I) and c.ld_a % 8 == 0 and c.ld_u % 8 == 0:
        return ("tr", c.O // 64, c.I // 32, bool(bits), bool(aux))
    assert not bits and not aux and c.O % 4 == 0 and c.I % 4 == 0 and c.ld_a % 4 == 0 and c.ld_u % 4 == 0
    return ("tiled",)


def wgrad_all_kernels():
    """Every instantiation the launcher can select: nine plain widths, the four masked ones, the two with the auxiliary rows, and the
    tiled kernel."""
    plain = {("tr", o, i, False, False) for o in (1, 2, 4) for i in (2, 4, 8)}
    masked = {("tr", o, i, True, False) for o in (2, 4) for i in (4, 8)}
    return plain | masked | {("tr", 4, 8, False, True), ("tr", 4, 8, True, True), ("tiled",)}


def exact_ints(n, d, what, lo=-8, hi=8):
    """[n, d] integers in [lo, hi]: bf16 values whose products and sums (below 2^24) are exact in fp32 in any order."""
    return torch.from_numpy(_rng("ints", what, n, d, lo, hi).integers(lo, hi + 1, size=(n, d)).astype(np.float64))


def wgrad_tables(n, O, I, kind):
    """ga [n, O], u [n, I] (bf16 values), g4 [n, 4] (fp32 values; the exact table's are bf16 values)."""
    if kind == "exact":
        return exact_ints(n, O, "ga"), exact_ints(n, I, "u"), exact_ints(n, 4, "g4")
    g4 = torch.from_numpy(_rng("g4", n).standard_normal((n, 4)).astype(np.float32)).double()
    return general_table(n, O, "wg-ga"), general_table(n, I, "wg-u"), g4


def wgrad_reference(ga, u, mask=None, g4=None):
    """gW = (ga * mask)^T u, gb = colsum(ga * mask) and, with g4, the auxiliary rows gWa = bf16(g4)^T u, gba = colsum(bf16(g4))."""
    a = ga if mask is None else ga * mask.double()
    out = [a.t() @ u, a.sum(0)]
    if g4 is not None:
        g16 = bf16_round(g4)
        out += [g16.t() @ u, g16.sum(0)]
    return out


REDUCE_CASES = [(P, M, M) for P in (1, 5, 64, 65, 700) for M in (8, 260)] + [(65, 260, 264)]     # (P, M, row stride)
RED_ROWS = 64                                            # dense.hip kRedRows


def reduce_is_tree(P, M):
    slabs = -(-P // RED_ROWS)
    return not (slabs == 1 or (slabs <= 8 and P * M <= 1 << 21))


def reduce_partials_table(P, stride, kind):
    """fp32 partials [P, stride]: integers in [-4000, 4000] (any partial sum below 2^24: exact in fp32), or randn."""
    r = _rng("partials", P, stride, kind)
    if kind == "exact":
        return torch.from_numpy(r.integers(-4000, 4001, size=(P, stride)).astype(np.float64))
    return torch.from_numpy(r.standard_normal((P, stride)).astype(np.float32)).double()


def truncate_bf16(ref):
    """float64 -> fp32 -> the bf16 below it in magnitude (``bits & 0xffff0000``), as float64."""
    return (ref.float().view(torch.int32) & -65536).view(torch.float32).double()


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
ADAM_CHUNK = 2048                                        # optim.hip kAdamChunk
ADAM_SIZES = (1, 2047, 2048, 0, 2049, 4097)              # a zero-element parameter between two others
ADAM_PRE_STEPS = (0, 1, 9, 999)
ADAM_WD = (0.0, 0.01)
ADAM_HYPER = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8)


def adam_sizes(max_tensors):
    """One more live parameter than a pointer table holds."""
    return list(ADAM_SIZES) + [5 + k for k in range(max_tensors + 1 - len(ADAM_SIZES))]


def _storage_round(t, bf16):
    return bf16_round(t) if bf16 else f32_round(t)


def adam_state(numel, bf16, what, wd_max=max(ADAM_WD)):
    """p = randn, g = +-10^U(-4, 2), exp_avg = +-10^U(-4, 2), exp_avg_sq = 10^U(-8, 2), all as the storage type holds them.
    Where g and wd * p would cancel to less than half of |wd * p| (at the largest weight decay of the cases) the sign of g is
    flipped: the bounds below budget the rounding of the product wd * p against |g + wd * p|."""
    r = _rng("adam", numel, bf16, what)
    sgn = lambda: np.where(r.integers(0, 2, size=numel) == 0, -1.0, 1.0)
    p = _storage_round(torch.from_numpy(r.standard_normal(numel)), bf16)
    g = _storage_round(torch.from_numpy(sgn() * 10.0 ** r.uniform(-4, 2, size=numel)), bf16)
    m = _storage_round(torch.from_numpy(sgn() * 10.0 ** r.uniform(-4, 2, size=numel)), bf16)
    v = _storage_round(torch.from_numpy(10.0 ** r.uniform(-8, 2, size=numel)), bf16)
    g = torch.where((g + wd_max * p).abs() < 0.5 * (wd_max * p).abs(), -g, g)
    return p, g, m, v


def adam_hyper32(lr, betas, eps, wd):
    """The hyper-parameters as the kernel receives them: rounded to float32."""
    return tuple(float(np.float32(v)) for v in (lr, betas[0], betas[1], eps, wd))


def adam_reference(p, g, m, v, t, lr, betas, eps, wd):
    """One step, float64, the header comment of csrc/optim.hip on the float32-rounded hyper-parameters; ``t`` = the step counter AFTER
    its increment.  Returns the new (p, m, v), the update ``delta`` (p_new = p - delta) and the magnitudes the moment bounds scale
    with: ``|b1 m| + |(1 - b1) g'|`` and ``|b2 v| + |(1 - b2) g'^2|``."""
    lr, b1, b2, eps, wd = adam_hyper32(lr, betas, eps, wd)
    gg = g + wd * p
    m2 = b1 * m + (1 - b1) * gg
    v2 = b2 * v + (1 - b2) * gg * gg
    delta = (lr / (1 - b1 ** t)) * m2 / (torch.sqrt(v2) / np.sqrt(1 - b2 ** t) + eps)
    return dict(p=p - delta, m=m2, v=v2, delta=delta, m_scale=(b1 * m).abs() + ((1 - b1) * gg).abs(),
                v_scale=(b2 * v).abs() + ((1 - b2) * gg * gg).abs(), p_old=p)


def adam_within(got, ref, which, bf16):
    """bool per element.  Moments: ``|got - ref| <= ulp_bf16(ref) / 2 + 2^-20 (|b old| + |(1 - b) new|)`` -- the kernel spends at most
    four fp32 roundings of 2^-24 on those terms (the rounding of ``g + wd p`` counts against ``new``, see ``adam_state``).  The
    parameter: ``ulp_bf16(ref) / 2 + 1e-4 |delta| + 2^-20 |p|`` -- ``1 - powf(b2, t)`` at t = 2, b2 = 0.999f carries 2^-23 / (1 - b2) =
    1.2e-4 relative, halved by the square root.  fp32 storage: the same without the ulp term."""
    got = got.detach().cpu().double()
    r = ref[which]
    assert got.shape == r.shape
    half = 0.5 * ulp_bf16(r) if bf16 else torch.zeros_like(r)
    if which == "p":
        tol = half + 1e-4 * ref["delta"].abs() + 2.0 ** -20 * ref["p_old"].abs()
    else:
        tol = half + 2.0 ** -20 * ref[which + "_scale"]
    return (got - r).abs() <= tol


def adam_half_ulps(got, ref, which):
    """max ``|got - ref| / (ulp/2)`` over |ref| >= 0.125 (reported)."""
    from bf16_cases import half_ulps, ROUNDING_GOVERNS
    return half_ulps(got, ref[which], ROUNDING_GOVERNS)


def assert_adam(got, ref, which, bf16, what):
    ok = adam_within(got, ref, which, bf16)
    if bf16:
        print(f"{what} {which}: max |got - ref| / (ulp/2) = {adam_half_ulps(got, ref, which):.4f} at |ref| >= 0.125")
    if not bool(ok.all()):
        i = int((~ok).nonzero()[0])
        raise AssertionError(f"{what} {which}: {int((~ok).sum())} of {ok.numel()} elements beyond the bound; first at {i}: got "
                             f"{float(got.detach().cpu().double().view(-1)[i])!r}, reference {float(ref[which].view(-1)[i])!r}")
