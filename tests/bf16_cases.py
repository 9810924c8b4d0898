"""The bf16 regime of the core aggregation surface (csrc/segreduce.hip, csrc/pma.hip): one row structure, the width and shape lists
that reach every bf16 instantiation of the two files, the input tables, their float64 references and the one acceptance rule.
Imports on the CPU; shared by tests/test_bf16_cases_host.py (which vouches for every case from float64 alone) and
tests/test_gpu_bf16_aggregate.py (which runs the same lists through the HIP kernels), so the two cannot drift.

A bf16 instantiation runs the fp32 instantiation's arithmetic and rounds ONCE, at the store.  Two kinds of table say that:
  * exact tables: ``x`` holds integers in [0, 16] (a signed copy in [-8, 8] for max / min), the incidence weights are drawn from
    {0.5, 1, 2, 4}.  Every product and every partial sum is a multiple of 0.5 below 2^24 * 0.5, exact in fp32 in ANY order, so the
    kernel's only rounding is the bf16 store and the expected BITS are ``float64 result -> .float() -> .bfloat16()`` (round to
    nearest even; the sums are ties on >= 10 % of the outputs and inexact on >= 50 %).  max / min also pin the arg-extremum array:
    the smallest CSR position among equal values (the integer tables tie on almost every column);
  * general tables: ``randn`` rounded to bf16 once, accepted by ``within_one_rounding`` against float64 on the same rounded values.
All values are float64 holding bf16- (tables, cotangents) or fp32- (weights, logits) representable numbers."""
from __future__ import annotations

import os
import sys
from collections import namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_structures as hs  # noqa: E402

D64 = torch.float64
SUM, MEAN, MAX, MIN = 0, 1, 2, 3                       # include/allset_hip.h ALLSET_SUM .. ALLSET_MIN (the GPU file pins them)
PACKET = 8                                             # bf16 elements in a 16-byte packet

# ---- the row structure ---------------------------------------------------------------------------------------------------------------
# Row lengths on both sides of the 64-incidence batch and of the NS * U unroll of the one-wave-per-row kernels (NS = 64 / LPR gathered
# rows per load, U = 8: 64 incidences per step at LPR = 8 ... 8 at LPR = 64), empty rows at the head, inside and near the tail.
N_SRC = 300
FIXED_LENGTHS = (0, 0, 1, 2, 3, 17, 63, 64, 65, 127, 128, 130, 300, 0, 1)
N_SMALL = 25                                           # small random rows behind them: 40 target rows
_STRUCT = {}


def structure():
    """``(n_src, n_dst, edge_index int64 [2, nnz] numpy)``: sources drawn WITH replacement (duplicates inside a row), the edge list
    shuffled (edge-list order is not CSR order)."""
    if "ei" not in _STRUCT:
        rng = np.random.default_rng(4101)
        lengths = list(FIXED_LENGTHS) + [int(v) for v in rng.integers(0, 8, size=N_SMALL)]
        src = np.concatenate([rng.integers(0, N_SRC, size=L) for L in lengths])
        dst = np.concatenate([np.full(L, t) for t, L in enumerate(lengths)])
        ei = np.stack([src, dst]).astype(np.int64)
        _STRUCT["ei"] = (N_SRC, len(lengths), ei[:, rng.permutation(ei.shape[1])])
    return _STRUCT["ei"]


Csr = namedtuple("Csr", "rowptr col perm n_rows n_cols")


def host_csr(flip=False):
    """The CSR ``ops.csr_build`` makes of the structure (a stable sort by target: ties keep the edge-list order), on the host:
    int64 numpy ``rowptr [n_rows + 1]``, ``col [nnz]``, ``perm [nnz]`` (CSR position -> edge-list position).  ``flip``: the
    transposed structure (rows = the 300 sources, short; columns = the 40 targets)."""
    key = ("csr", flip)
    if key not in _STRUCT:
        n_src, n_dst, ei = structure()
        rows, cols, n_rows, n_cols = (ei[0], ei[1], n_src, n_dst) if flip else (ei[1], ei[0], n_dst, n_src)
        perm = np.argsort(rows, kind="stable")
        rowptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_rows))]).astype(np.int64)
        _STRUCT[key] = Csr(rowptr, cols[perm].astype(np.int64), perm.astype(np.int64), n_rows, n_cols)
    return _STRUCT[key]


def edges(flip=False):
    """int64 tensor [2, nnz] (row 0 gathered rows, row 1 output rows) of the structure or of its transpose."""
    ei = torch.from_numpy(structure()[2])
    return torch.stack([ei[1], ei[0]]) if flip else ei


# ---- widths and shapes ---------------------------------------------------------------------------------------------------------------
SegWidth = namedtuple("SegWidth", "id d pitch")
# d: 16-byte packets on 8 / 16 / 32 / 64 lanes; 520: 64 lanes, two column chunks; 20 / 70: the scalar path, one / two chunks; 64 in a
# buffer of row pitch 68: the scalar path through the leading dimension alone
SEG_WIDTHS = [SegWidth(f"d{d}", d, d) for d in (64, 128, 256, 512, 520, 20, 70)] + [SegWidth("d64p68", 64, 68)]
FLAT_WIDTHS = [w for w in SEG_WIDTHS if w.pitch == w.d and w.d in (64, 128, 256, 512)]       # variant 2: sum / mean
BWD_WIDTHS = (20, 70, 128, 512)

PmaShape = namedtuple("PmaShape", "id H C variant")
PMA_SCALAR = [(3, 4), (1, 20), (2, 36)]                                   # (2, 36): two scalar column chunks
PMA_WAVE = [(1, 64), (4, 32), (8, 32), (8, 64), (1, 520)]                 # pick_lpr(H * C, 8) = 8 / 16 / 32 / 64; (1, 520): two packet chunks
PMA_FLAT = [(2, 32), (4, 32), (4, 64), (4, 72), (8, 64)]                  # LPR 8 / 16 / 32 / 64 (H * C = 288) / 64 (512)
PMA_SHAPES = ([PmaShape(f"H{H}C{C}-v1", H, C, 1) for H, C in PMA_SCALAR + PMA_WAVE] +
              [PmaShape(f"H{H}C{C}-v2", H, C, 2) for H, C in PMA_FLAT])
PMA_SLOPE = 0.2


def seg_geometry(w, variant=1):
    """``(kernel, VEC, LPR, column chunks)`` that ``segreduce_impl`` reaches for contiguous 16-byte aligned bf16 buffers of this width
    and pitch (csrc/segreduce.hip, with_vec_lpr / pick_lpr of csrc/flat_rows.h and csrc/common.h restated)."""
    wide_ok = w.d % PACKET == 0 and w.pitch % PACKET == 0
    if variant == 2:
        assert wide_ok and w.d <= 64 * PACKET
        return "flat", PACKET, hs.pick_lpr(w.d, PACKET), 1
    vec, lpr = (PACKET, hs.pick_lpr(w.d, PACKET)) if wide_ok else (1, 64)
    return "wave", vec, lpr, -(-w.d // (vec * lpr))


def pma_geometry(s):
    """The same for ``pma_fwd_impl`` / ``pma_bwd_src_impl``: 16-byte packets need ``C % 8 == 0``."""
    d = s.H * s.C
    wide_ok = s.C % PACKET == 0
    if s.variant == 2:
        assert wide_ok and d <= 64 * PACKET
        return "flat", PACKET, hs.pick_lpr(d, PACKET), 1
    vec, lpr = (PACKET, hs.pick_lpr(d, PACKET)) if wide_ok else (1, 64)
    return "wave", vec, lpr, -(-d // (vec * lpr))


def pma_stats_geometry(s):
    """``pma_bwd_stats_impl`` has no variant: every packet-aligned row of at most 64 packets takes the slot-per-row kernel."""
    d = s.H * s.C
    if s.C % PACKET == 0 and d <= 64 * PACKET:
        return "flat", PACKET, hs.pick_lpr(d, PACKET), 1
    vec, lpr = (PACKET, 64) if s.C % PACKET == 0 else (1, 64)
    return "wave", vec, lpr, -(-d // (vec * lpr))


# ---- tables --------------------------------------------------------------------------------------------------------------------------
def bf16_round(t):
    """float64 -> the float64 holding its bf16 rounding (through fp32: exact for every value here, see the host file)."""
    return t.float().bfloat16().double()


def _rng(*parts):
    return np.random.default_rng(hs.hash_id("-".join(str(p) for p in parts)))


def exact_table(d, signed=False):
    """[N_SRC, d] integers in [0, 16], or in [-8, 8] (max / min: both signs, ties on almost every column)."""
    v = _rng("exact", d, signed).integers(0, 17, size=(N_SRC, d))
    return torch.from_numpy((v - 8 if signed else v).astype(np.float64))


def exact_weights():
    """Per incidence in EDGE-LIST order, from {0.5, 1, 2, 4}."""
    nnz = structure()[2].shape[1]
    return torch.from_numpy(_rng("exact-w").choice([0.5, 1.0, 2.0, 4.0], size=nnz))


def general_table(n, d, what="x"):
    """``randn`` rounded to bf16 once."""
    return bf16_round(torch.from_numpy(_rng("general", what, n, d).standard_normal((n, d))))


def general_weights():
    """fp32 values in [0.5, 1.5), edge-list order."""
    nnz = structure()[2].shape[1]
    return torch.from_numpy((_rng("general-w").random(nnz) + 0.5).astype(np.float32)).double()


def logits(n, H, what):
    """fp32 multiples of 1/8 in [-2, 2] plus 1/16 (``hop_structures.logit_terms``): at least 1/16 from leaky_relu's kink."""
    return hs.logit_terms(_rng("logits", what, n, H), n, H, True)


# ---- float64 references --------------------------------------------------------------------------------------------------------------
def seg_reference(reduce, x, w_edge=None, flip=False):
    """``(out float64 [n_rows, d], argext int32 [n_rows, d] or None)`` over the host CSR.  Empty rows: 0 and -1.  max / min: the
    SMALLEST CSR position among equal extremal values (numpy's argmax / argmin return the first)."""
    csr = host_csr(flip)
    xn = x.numpy()
    w = None if w_edge is None else w_edge.numpy()[csr.perm]
    out = np.zeros((csr.n_rows, xn.shape[1]))
    arg = np.full((csr.n_rows, xn.shape[1]), -1, dtype=np.int32) if reduce in (MAX, MIN) else None
    for t in range(csr.n_rows):
        a, b = int(csr.rowptr[t]), int(csr.rowptr[t + 1])
        if a == b:
            continue
        vals = xn[csr.col[a:b]] if w is None else xn[csr.col[a:b]] * w[a:b, None]
        if reduce in (SUM, MEAN):
            out[t] = vals.sum(0) / (b - a if reduce == MEAN else 1)
        else:
            k = vals.argmax(0) if reduce == MAX else vals.argmin(0)
            out[t] = np.take_along_axis(vals, k[None], 0)[0]
            arg[t] = a + k
    return torch.from_numpy(out), (None if arg is None else torch.from_numpy(arg))


def row_lengths(flip=False):
    csr = host_csr(flip)
    return np.diff(csr.rowptr)


_PMA_REF = {}


def pma_reference(H, C, flip):
    """Everything the three PMA entries are held to, once per (shape, orientation), float64, from ``oracle.pma_aggregate`` on the
    bf16-rounded ``V`` and cotangent ``G`` (backward: autograd):
      V [n_s, H*C], alpha [n_s, H] (fp32 logits), G [n_t, H*C];
      out [n_t, H*C], m / l [n_t, H] (row maximum of the activated logits / sum of exp(a - m); both 0 on an empty row),
      stats [n_t, H, 2] = (m + log(l + 1e-16), <out[t, h], G[t, h]>); ``empty`` bool [n_t]: the rows without incidence, where the kernel
      stores FLT_MAX for the first entry; gV [n_s, H*C], galpha [n_s, H]."""
    key = (H, C, flip)
    if key in _PMA_REF:
        return _PMA_REF[key]
    from oracle import allset_oracle as oracle
    ei = edges(flip)
    csr = host_csr(flip)
    n_s, n_t, d = csr.n_cols, csr.n_rows, H * C
    V = general_table(n_s, d, f"V{flip}")
    G = general_table(n_t, d, f"G{flip}")
    alpha = logits(n_s, H, f"alpha{flip}")
    Vl, al = V.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    out, _ = oracle.pma_aggregate(Vl.view(n_s, H, C), al, ei, PMA_SLOPE)
    out = out.reshape(-1, d)
    out = torch.cat([out, out.new_zeros(n_t - out.shape[0], d)])
    (out * G).sum().backward()
    a = torch.nn.functional.leaky_relu(alpha, PMA_SLOPE)[ei[0]]
    idx = ei[1].view(-1, 1).expand(-1, H)
    m = torch.full((n_t, H), -float("inf"), dtype=D64).scatter_reduce(0, idx, a, "amax", include_self=True)
    empty = torch.from_numpy(np.diff(csr.rowptr) == 0)
    m[empty] = 0.0
    l = torch.zeros((n_t, H), dtype=D64).scatter_add(0, idx, torch.exp(a - m[ei[1]]))
    out = out.detach()
    stats = torch.stack([m + torch.log(l + 1e-16), (out.view(n_t, H, C) * G.view(n_t, H, C)).sum(-1)], dim=-1)
    ref = dict(n_s=n_s, n_t=n_t, V=V, alpha=alpha, G=G, out=out, m=m, l=l, stats=stats, empty=empty, gV=Vl.grad, galpha=al.grad)
    _PMA_REF[key] = ref
    return ref


def pma_stats_reference(out_b, G, m, l, H):
    """``pma_bwd_stats`` on ITS inputs (the stored bf16 ``out`` -- not the unrounded one -- the cotangent and the fp32 ``m`` / ``l``),
    float64: [n_t, H, 2]."""
    n_t = out_b.shape[0]
    return torch.stack([m + torch.log(l + 1e-16), (out_b.view(n_t, H, -1) * G.view(n_t, H, -1)).sum(-1)], dim=-1)


# ---- the acceptance rule -------------------------------------------------------------------------------------------------------------
FP32_TOL = 1e-4                                        # tests/test_gpu_ops.py RTOL = ATOL: what the same arithmetic is held to in fp32


def ulp_bf16(ref):
    """2^(floor(log2 |r|) - 7): the spacing of bf16 (8 significant bits) at ``r``; 0 at 0."""
    a = ref.abs()
    e = torch.floor(torch.log2(torch.where(a > 0, a, torch.ones_like(a))))
    return torch.where(a > 0, torch.exp2(e - 7), torch.zeros_like(a))


def within_one_rounding(got, ref):
    """bool per element: ``|got - ref| <= 1/2 ulp_bf16(ref) + 1e-4 |ref| + 1e-4`` -- the one permitted rounding on top of the fp32
    kernels' own tolerance."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} against {tuple(ref.shape)}"
    return (got - ref).abs() <= 0.5 * ulp_bf16(ref) + FP32_TOL * ref.abs() + FP32_TOL


ROUNDING_GOVERNS = 0.125                               # |ref| from which 1/2 ulp (>= 2^-11) is over four times the rule's fp32 terms (<= 1.13e-4)


def half_ulps(got, ref, floor=0.0):
    """max ``|got - ref| / (1/2 ulp_bf16(ref))`` over the elements with ``|ref| >= floor`` and a non-zero reference (reported, not
    asserted).  Near a zero of the reference the figure is the fp32 error of a cancelling sum over a vanishing ulp and says nothing
    about the rounding: ``floor = ROUNDING_GOVERNS`` leaves those out."""
    got = got.detach().cpu().double()
    nz = (ref != 0) & (ref.abs() >= floor)
    return float(((got - ref).abs()[nz] / (0.5 * ulp_bf16(ref)[nz])).max()) if bool(nz.any()) else 0.0


def assert_one_rounding(got, ref, what):
    ok = within_one_rounding(got, ref)
    worst = half_ulps(got, ref)
    print(f"{what}: max |got - ref| / (ulp/2) = {half_ulps(got, ref, ROUNDING_GOVERNS):.4f} at |ref| >= {ROUNDING_GOVERNS}, {worst:.4f} "
          f"anywhere; max |ref| {float(ref.abs().max()) if ref.numel() else 0.0:.3e}")
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(int(v) for v in bad[0])
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements beyond one bf16 rounding; first at {i}: got "
                             f"{float(got.detach().cpu().double()[i])!r}, reference {float(ref[i])!r}, ulp {float(ulp_bf16(ref)[i])!r}; "
                             f"max |got - ref| / (ulp/2) = {worst:.3f}")


close_fp32 = hs.close      # the fp32 outputs (m, l, stats, galpha): rtol 1e-4, atol 1e-4 * max(1, max |ref|), the sparse-hop sweep's rule


def bits_equal(got_bf16, want_bf16):
    """bool per element: the same bf16 bits, +0 and -0 taken as equal."""
    g, w = got_bf16.detach().cpu(), want_bf16.detach().cpu()
    return (g.view(torch.int16) == w.view(torch.int16)) | ((g.float() == 0) & (w.float() == 0))
