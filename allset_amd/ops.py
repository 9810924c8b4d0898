"""Thin tensor-level wrappers over the C ABI (one python function per entry point of
``include/allset_hip.h``).  No autograd here -- see ``functional.py``.  All tensors are ROCm device
tensors; outputs are allocated with torch (plumbing) and filled by the HIP kernels.
"""
from __future__ import annotations

from collections import defaultdict
from ctypes import byref, c_int64 as c_int64_t, c_size_t, c_void_p
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import _lib
from ._lib import check, ptr, require_device, stream_of, on_device

Tensor = torch.Tensor


class KernelTimer:
    """Opt-in per-entry-point timing with HIP events recorded on the stream the kernels are launched on
    (torch's current stream).  ``bench.py`` installs one over its timed region; when none is installed
    the wrappers below add no events.  ``algo_bytes`` is the ALGORITHMIC traffic of the call (SURVEY.md
    section 8(d3) gather model: every incidence reads its d-vector once; int32 CSR)."""

    def __init__(self):
        self.events: Dict[str, List[Tuple[torch.cuda.Event, torch.cuda.Event, int]]] = defaultdict(list)

    def summary(self) -> Dict[str, Dict[str, float]]:
        """Call after a device synchronise.  name -> {calls, avg_ms, total_ms, algo_bytes (per call)}."""
        out = {}
        for name, evs in self.events.items():
            ms = [s.elapsed_time(e) for s, e, _ in evs]
            out[name] = dict(calls=len(ms), total_ms=sum(ms), avg_ms=sum(ms) / len(ms),
                             algo_bytes=sum(b for _, _, b in evs) / len(evs))
        return out


_timer: Optional[KernelTimer] = None


def set_kernel_timer(timer: Optional[KernelTimer]) -> None:
    global _timer
    _timer = timer


class _NoTimer:
    """Shared do-nothing context: the common case (no KernelTimer installed) must cost nothing per launch."""
    __slots__ = ()

    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NO_TIMER = _NoTimer()


class _Timed:
    __slots__ = ("t", "name", "st", "s", "bytes")

    def __init__(self, t, name, dev, algo_bytes):
        self.t, self.name, self.bytes = t, name, int(algo_bytes)
        self.st = torch.cuda.current_stream(dev)

    def __enter__(self):
        self.s = torch.cuda.Event(enable_timing=True)
        self.s.record(self.st)
        return None

    def __exit__(self, *exc):
        e = torch.cuda.Event(enable_timing=True)
        e.record(self.st)
        self.t.events[self.name].append((self.s, e, self.bytes))
        return False


def _timed(name: str, dev, algo_bytes: int):
    t = _timer
    return _NO_TIMER if t is None else _Timed(t, name, dev, algo_bytes)


class SizeSplit(NamedTuple):
    """A skewed CSR cut by row length (round 3): the few LONG rows (> ``threshold`` incidences) as a list for
    the one-wave-per-row kernels, the many SHORT rows as a compacted CSR (+ their ids) for the short-row kernels, which pack
    64 / LPR rows into a wave.  Pays where a row is at most one cache line (the column-sharded PMA layer: d / P columns): one wave
    per row leaves most lanes idle there, and the short-row kernels alone would serialise a 4096-member row in one lane group."""
    long_ids: Tensor          # int32[n_long]
    short_ids: Tensor         # int32[n_short]
    rowptr_short: Tensor      # int32[n_short + 1] into col_short
    col_short: Tensor         # int32[nnz_short]
    threshold: int


SIZE_SPLIT_THRESHOLD = int(__import__('os').environ.get('ALLSET_SIZE_SPLIT_T', '32'))      # (env: tuning sweeps only)


def size_split(rowptr: Tensor, col: Tensor, n_rows: int, max_deg: int, threshold: int = SIZE_SPLIT_THRESHOLD) -> Optional[SizeSplit]:
    """Built once per CSR (one host sync), only for skewed row lengths: some row longer than ``threshold`` and at most 1/8 of the
    rows long."""
    if n_rows <= 0 or max_deg <= threshold or col.numel() == 0:
        return None
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    is_long = deg > threshold
    n_long = int(is_long.sum())
    if n_long == 0 or n_long * 8 > n_rows:
        return None
    long_ids = is_long.nonzero().reshape(-1).to(torch.int32)
    short_ids64 = (~is_long).nonzero().reshape(-1)
    deg_s = deg[short_ids64]
    rowptr_short = torch.zeros(short_ids64.numel() + 1, dtype=torch.int32, device=rowptr.device)
    rowptr_short[1:] = torch.cumsum(deg_s, 0).to(torch.int32)
    keep = ~torch.repeat_interleave(is_long, deg)                  # per incidence: its row is short
    return SizeSplit(long_ids, short_ids64.to(torch.int32), rowptr_short, col[keep].contiguous(), threshold)


class CSR(NamedTuple):
    """rowptr int32[n_rows+1], col int32[nnz], perm int32[nnz] (CSR position -> edge-list position);
    ``max_deg`` = longest row (read back once when the CSR is built; used to pick kernel variants)."""
    rowptr: Tensor
    col: Tensor
    perm: Tensor
    n_rows: int
    n_cols: int
    max_deg: int = 0
    row_order: Optional[Tensor] = None      # int32[n_rows] processing order (long rows first per XCD range) or None
    short_tail: int = -1                    # rows >= short_tail all have <= 2 incidences (Add_Self_Loops' singleton
                                            # hyperedges sit at the end of the id range) and are worth their own launch
    sizes: Optional[SizeSplit] = None       # skewed row lengths: long-row list + compacted short rows (narrow-row PMA kernels)

    def variant(self, kind: str, n_rows: Optional[int] = None) -> int:
        """Kernel variant for this orientation: 2 = short-row kernel, 1 = one wavefront per row.  Thresholds from
        profiles/r01_kernel_bench*.txt: the short-row kernels win below a mean degree of ~6 (segreduce, pma_fwd) and
        up to ~24 for pma_bwd_src, as long as no row is long enough to serialise a half-wave."""
        rows = max(int(self.n_rows if n_rows is None else n_rows), 1)
        if kind == "segreduce" and rows <= 16384:
            # dataset scale: every row gets its own lane group on a machine this size; the one-group-per-row kernel is one dependent
            # round trip shorter than a slot walking seven rows as a stream (the same rule as the library's AUTO, kFlatMinRows)
            return 1
        mean = self.col.numel() / rows
        limit = 24.0 if kind == "pma_bwd_src" else 6.0
        return 2 if (mean < limit and self.max_deg <= 512) else 1

    @property
    def nnz(self) -> int:
        return int(self.col.numel())


def _rowmajor(t: Tensor) -> Tensor:
    """Kernels take row-major matrices with an explicit leading dimension (stride(1) == 1)."""
    if t.dim() != 2:
        raise _lib.AllSetHipError(f"expected a 2-D matrix, got shape {tuple(t.shape)}")
    if t.shape[1] > 1 and t.stride(1) != 1 or t.stride(0) < t.shape[1]:
        return t.contiguous()
    return t


def _ld(t: Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else max(t.shape[1], 1)


def _f32(t: Tensor, what: str) -> None:
    if t.dtype != torch.float32:
        raise _lib.AllSetHipError(f"{what}: float32 required (got {t.dtype})")


def _dtype_code(t: Tensor, what: str) -> int:
    """Storage dtype of a feature matrix: fp32, or bf16 (accumulation is fp32 in both cases)."""
    if t.dtype == torch.float32:
        return _lib.F32
    if t.dtype == torch.bfloat16:
        return _lib.BF16
    raise _lib.AllSetHipError(f"{what}: float32 or bfloat16 storage required (got {t.dtype})")


def csr_build(row_ids: Tensor, col_ids: Tensor, row_base: int, col_base: int, n_rows: int, n_cols: int) -> CSR:
    dev = require_device(row_ids, col_ids)
    if row_ids.dtype != torch.int64 or col_ids.dtype != torch.int64:
        raise _lib.AllSetHipError("csr_build: int64 ids required (the reference's edge_index dtype)")
    row_ids, col_ids = row_ids.contiguous(), col_ids.contiguous()
    nnz = row_ids.numel()
    lib = _lib.load()
    need = c_size_t(0)
    with on_device(dev):
        check(lib.allset_csr_build_workspace_bytes(nnz, n_rows, byref(need)), "allset_csr_build_workspace_bytes")
        rowptr = torch.empty(n_rows + 1, dtype=torch.int32, device=dev)
        col = torch.empty(nnz, dtype=torch.int32, device=dev)
        perm = torch.empty(nnz, dtype=torch.int32, device=dev)
        ws = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)   # caching allocator: 512-B aligned
        check(lib.allset_csr_build(ptr(row_ids), ptr(col_ids), nnz, row_base, col_base, n_rows,
                                   ptr(rowptr), ptr(col), ptr(perm), ptr(ws), need.value, stream_of(dev)),
              "allset_csr_build")
    max_deg, short_tail = 0, -1
    if n_rows > 0 and nnz > 0:                                                            # one-time sync at build
        deg = rowptr[1:] - rowptr[:-1]
        big = (deg > 2).nonzero()
        stats = torch.stack([deg.max().to(torch.int64), (big[-1, 0] + 1) if big.numel() else torch.zeros((), dtype=torch.int64, device=dev)])
        max_deg, first_short = (int(v) for v in stats.tolist())
        head_nnz = int(rowptr[first_short]) if first_short > 0 else 0
        # a block of singleton rows behind regular rows (the reference's default Add_Self_Loops layout): one wave per
        # row wastes the launch on them, the short-row kernel wastes the long rows -- give each block its kernel
        if 0 < first_short < n_rows and (n_rows - first_short) * 16 >= n_rows and head_nnz >= 6 * first_short and max_deg <= 100000:
            short_tail = first_short
    return CSR(rowptr, col, perm, n_rows, n_cols, max_deg, long_rows_first_order(rowptr, n_rows, nnz, max_deg), short_tail,
               size_split(rowptr, col, n_rows, max_deg) if short_tail < 0 else None)


def long_rows_first_order(rowptr: Tensor, n_rows: int, nnz: int, max_deg: int) -> Optional[Tensor]:
    """Processing order for skewed degree distributions, or None when the distribution is not skewed.

    The one-wave-per-row kernels map workgroup b to XCD b % 8 and give every XCD a contiguous range of row slots.
    A row with thousands of incidences keeps one wave busy for ~0.3 ms; if it is dispatched late it sets the end
    of the launch (profiles: Zipf sizes up to 4096 run at 80 % of the uniform-size rate).  This permutation lists,
    for each XCD's slot range, that XCD's share of the long rows first (round-robin, longest first) and then the
    remaining rows in natural order -- the results are unchanged, only the dispatch order moves."""
    if n_rows < 64 or nnz == 0:
        return None
    mean = nnz / n_rows
    if not (max_deg > 256 and max_deg > 8.0 * mean):
        return None
    dev = rowptr.device
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    long_mask = deg > max(64, int(4 * mean))
    long_rows = long_mask.nonzero().reshape(-1)
    if long_rows.numel() == 0 or long_rows.numel() > n_rows // 4:
        return None
    long_rows = long_rows[torch.argsort(deg[long_rows], descending=True, stable=True)]
    rest = (~long_mask).nonzero().reshape(-1)
    nb = (n_rows + 3) // 4                                   # workgroups (4 rows each)
    q, r = nb // 8, nb % 8
    order = torch.empty(n_rows, dtype=torch.int64, device=dev)
    slot, taken = 0, 0
    for xcd in range(8):
        cnt = min(4 * (q + 1 if xcd < r else q), n_rows - slot)      # row slots of this XCD
        mine = long_rows[xcd::8]
        k = int(mine.numel())
        if k > cnt:
            return None                                        # more long rows than slots: not a skew problem
        order[slot:slot + k] = mine
        order[slot + k:slot + cnt] = rest[taken:taken + cnt - k]
        taken += cnt - k
        slot += cnt
    if slot != n_rows or taken != rest.numel():
        return None
    return order.to(torch.int32).contiguous()


def segreduce(reduce: int, rowptr: Tensor, col: Tensor, w: Optional[Tensor], x: Tensor, n_t: int,
              want_arg: bool = False, variant: int = 0, row_order: Optional[Tensor] = None, split: int = -1
              ) -> Tuple[Tensor, Optional[Tensor]]:
    """``variant``: 0 auto (short-row kernel when nnz / n_t < 6), 1 one wave per row, 2 short-row kernel.
    ``split`` (``CSR.short_tail``): rows >= split go to the short-row kernel in a second launch."""
    dev = require_device(rowptr, col, w, x)
    code = _dtype_code(x, "segreduce")
    es = x.element_size()
    x = _rowmajor(x)
    n_s, d = x.shape
    out = torch.empty((n_t, d), dtype=x.dtype, device=dev)
    arg = torch.empty((n_t, d), dtype=torch.int32, device=dev) if want_arg else None
    if w is not None:
        _f32(w, "segreduce weights")
        w = w.contiguous()
    nnz = col.numel()
    algo = nnz * (es * d + 4 + (4 if w is not None else 0)) + (n_t + 1) * 4 + n_t * d * es
    with on_device(dev), _timed("segreduce_fwd", dev, algo):
        if row_order is not None and row_order.numel() != n_t:
            row_order = None                       # order was built for a different row count (prefix views)
        lib = _lib.load()
        if 0 < split < n_t and not want_arg and rowptr.numel() == n_t + 1:
            # regular rows: one wave per row; the singleton tail: short-row kernel (same rowptr / col / out buffers, the
            # row pointers are absolute positions so an offset view is all the second launch needs)
            check(lib.allset_segreduce_fwd_ex(reduce, code, 1, nnz, None, ptr(rowptr), ptr(col), ptr(w), ptr(x), _ld(x),
                                              ptr(out), max(d, 1), None, split, n_s, d, stream_of(dev)), "allset_segreduce_fwd_ex")
            check(lib.allset_segreduce_fwd_ex(reduce, code, 2, nnz, None, ptr(rowptr[split:]), ptr(col), ptr(w), ptr(x), _ld(x),
                                              ptr(out[split:]), max(d, 1), None, n_t - split, n_s, d, stream_of(dev)),
                  "allset_segreduce_fwd_ex")
        else:
            check(lib.allset_segreduce_fwd_ex(reduce, code, variant, nnz, ptr(row_order), ptr(rowptr), ptr(col), ptr(w), ptr(x), _ld(x),
                                              ptr(out), max(d, 1), ptr(arg), n_t, n_s, d, stream_of(dev)),
                  "allset_segreduce_fwd_ex")
    return out, arg


# The two packed-row formats of the forward Deep Sets gather (include/allset_hip_ext.h): "mask" rows (a 128-bit
# occupancy mask + the occupied elements) and "cells" rows (16 cells of three elements with their columns and the row's count).  Per
# format: the occupied columns a row holds (a row above ``cap`` is read from the dense table instead) and its C entry points -- the pack
# pass, the gather, the fused Linear that writes the rows from its epilogue and that Linear's ``_supported`` query.  Everything that
# takes a format name looks it up here (:func:`packed_format_entry`).
PACKED_FORMATS = {
    "mask": dict(cap=_lib.PACK_CAP, pack="allset_pack_rows_f32", gather="allset_segreduce_packed_fwd",
                 linear="allset_fused_linear_fwd_packed", supported="allset_fused_linear_fwd_packed_supported"),
    "cells": dict(cap=_lib.CELL_CAP, pack="allset_pack_cells_f32", gather="allset_segreduce_cells_fwd",
                  linear="allset_fused_linear_fwd_cells", supported="allset_fused_linear_fwd_cells_supported"),
}


def packed_format_entry(fmt: str, who: str) -> dict:
    """The table entry of ``fmt``; anything else is a ``ValueError`` in ``who``'s name."""
    if not isinstance(fmt, str) or fmt not in PACKED_FORMATS:
        raise ValueError(f"{who}: format must be {' or '.join(repr(k) for k in PACKED_FORMATS)}, got {fmt!r}")
    return PACKED_FORMATS[fmt]


def pack_rows(x: Tensor, *, fmt: str) -> Tensor:
    """``x`` f32[n, 128] -> int32[n, 64]: every row in the packed format ``fmt`` (:data:`PACKED_FORMATS`).  One streaming pass, no sync."""
    sym = packed_format_entry(fmt, "pack_rows")["pack"]
    dev = require_device(x)
    _f32(x, "pack_rows")
    x = _rowmajor(x)
    n, d = x.shape
    packed = torch.empty((n, _lib.PACK_PITCH_DW), dtype=torch.int32, device=dev)
    with on_device(dev), _timed("pack_rows", dev, n * (4 * d + 4 * _lib.PACK_PITCH_DW)):
        check(getattr(_lib.load(), sym)(ptr(x), _ld(x), ptr(packed), n, d, stream_of(dev)), sym)
    return packed


def fused_linear_fwd_packed_supported(K: int, N: int, has_ln: bool, p_in: float, p_out: float, *, fmt: str) -> bool:
    sym = packed_format_entry(fmt, "fused_linear_fwd_packed_supported")["supported"]
    return bool(getattr(_lib.load(), sym)(int(K), int(N), int(has_ln), float(p_in), float(p_out)))


def fused_linear_fwd_packed(x: Tensor, weight: Tensor, bias: Optional[Tensor], gamma: Tensor, beta: Tensor, eps: float, relu_in: bool,
                            p_in: float, seed_in: int, relu_out: bool, p_out: float, seed_out: int, seed_base: Optional[Tensor],
                            mask_out: Optional[Tensor], arith: int = 0, *, fmt: str) -> Tuple[Tensor, Tensor, Tensor]:
    """The fused Linear forward (``dense.fused_linear_fwd`` behind a LayerNorm, dropout in and out) with ``pack_rows(., fmt=fmt)`` as its
    epilogue: returns ``(packed int32[n, 64], side f32[n, N], stats)``.  ``side`` is UNINITIALISED except for the rows above the format's
    capacity -- (packed, side) is what :func:`segreduce_packed` takes as (packed, x), and nothing else may read ``side``."""
    sym = packed_format_entry(fmt, "fused_linear_fwd_packed")["linear"]
    dev = require_device(x, weight, bias, gamma, beta)
    for t in (x, weight, bias, gamma, beta):
        if t is not None:
            _f32(t, "fused_linear_fwd_packed")
    x = _rowmajor(x)
    n, K = x.shape
    N = weight.shape[0]
    packed = torch.empty((n, _lib.PACK_PITCH_DW), dtype=torch.int32, device=dev)
    side = torch.empty((n, N), dtype=torch.float32, device=dev)
    stats = torch.empty((n, 2), dtype=torch.float32, device=dev)
    nparam = weight.numel() + N + 2 * K
    with on_device(dev), _timed("fused_linear_fwd", dev, n * (4 * K + 4 * _lib.PACK_PITCH_DW) + 4 * nparam):
        check(getattr(_lib.load(), sym)(
            ptr(x), _ld(x), ptr(gamma.contiguous()), ptr(beta.contiguous()), eps, int(relu_in), p_in, seed_in, ptr(weight.contiguous()),
            ptr(bias.contiguous() if bias is not None else None), int(relu_out), p_out, seed_out, ptr(packed), ptr(side), max(N, 1),
            ptr(stats), n, K, N, ptr(seed_base), ptr(mask_out), int(arith), stream_of(dev)), sym)
    return packed, side, stats


def segreduce_packed(reduce: int, rowptr: Tensor, col: Tensor, packed: Tensor, x: Tensor, n_t: int,
                     row_order: Optional[Tensor] = None, *, fmt: str) -> Tensor:
    """``segreduce(reduce, rowptr, col, None, x, n_t, variant=1, row_order=row_order)[0]``, bit for bit, gathering
    ``packed = pack_rows(x, fmt=fmt)`` (two lines per row instead of four); ``x`` itself is read only for rows above the format's
    capacity.  SUM / MEAN, fp32, d = 128."""
    sym = packed_format_entry(fmt, "segreduce_packed")["gather"]
    dev = require_device(rowptr, col, packed, x)
    _f32(x, "segreduce_packed")
    x = _rowmajor(x)
    n_s, d = x.shape
    if packed.dtype != torch.int32 or tuple(packed.shape) != (n_s, _lib.PACK_PITCH_DW) or not packed.is_contiguous():
        raise _lib.AllSetHipError(f"segreduce_packed: packed must be contiguous int32[{n_s}, {_lib.PACK_PITCH_DW}] (ops.pack_rows)")
    out = torch.empty((n_t, d), dtype=x.dtype, device=dev)
    nnz = col.numel()
    algo = nnz * (4 * _lib.PACK_PITCH_DW + 4) + (n_t + 1) * 4 + n_t * d * 4
    with on_device(dev), _timed("segreduce_fwd", dev, algo):
        if row_order is not None and row_order.numel() != n_t:
            row_order = None                       # order was built for a different row count (prefix views)
        check(getattr(_lib.load(), sym)(reduce, ptr(row_order), ptr(rowptr), ptr(col), ptr(packed), ptr(x), _ld(x),
                                        ptr(out), max(d, 1), n_t, n_s, d, stream_of(dev)), sym)
    return out


def segmax_bwd(rowptrT: Tensor, colT: Tensor, posT: Tensor, wT: Optional[Tensor], argext: Tensor, gout: Tensor,
               n_s: int) -> Tensor:
    dev = require_device(rowptrT, colT, posT, wT, argext, gout)
    _f32(gout, "segmax_bwd")
    gout = _rowmajor(gout)
    n_t, d = gout.shape
    if colT.numel() == 0:                       # no incidences: no row received anything (the ABI takes no null index arrays)
        return torch.zeros((n_s, d), dtype=gout.dtype, device=dev)
    gx = torch.empty((n_s, d), dtype=gout.dtype, device=dev)
    algo = colT.numel() * (4 * d + 4 * d + 8) + (n_s + 1) * 4 + n_s * d * 4
    with on_device(dev), _timed("segmax_bwd", dev, algo):
        check(_lib.load().allset_segmax_bwd(ptr(rowptrT), ptr(colT), ptr(posT), ptr(wT), ptr(argext), ptr(gout),
                                            _ld(gout), ptr(gx), max(d, 1), n_s, n_t, d, stream_of(dev)),
              "allset_segmax_bwd")
    return gx


def sddmm_rowdot(reduce: int, rowptr: Tensor, col: Tensor, x: Tensor, gout: Tensor, argext: Optional[Tensor]) -> Tensor:
    dev = require_device(rowptr, col, x, gout, argext)
    _f32(x, "sddmm_rowdot")
    x, gout = _rowmajor(x), _rowmajor(gout)
    n_s, d = x.shape
    n_t = gout.shape[0]
    gw = torch.empty(col.numel(), dtype=torch.float32, device=dev)
    if col.numel() == 0:
        return gw
    algo = col.numel() * (4 * d + 8) + (n_t + 1) * 4 + n_t * d * 4
    with on_device(dev), _timed("sddmm_rowdot", dev, algo):
        check(_lib.load().allset_sddmm_rowdot(reduce, ptr(rowptr), ptr(col), ptr(x), _ld(x), ptr(gout), _ld(gout),
                                              ptr(argext), ptr(gw), n_t, n_s, d, stream_of(dev)),
              "allset_sddmm_rowdot")
    return gw


def pma_fwd(rowptr: Tensor, col: Tensor, alpha: Tensor, V: Tensor, heads: int, slope: float, n_t: int,
            variant: int = 0, row_order: Optional[Tensor] = None, split: int = -1, sizes: Optional[SizeSplit] = None
            ) -> Tuple[Tensor, Tensor, Tensor]:
    """``sizes`` (``CSR.sizes``): two launches -- the long rows one wave each, the short rows through the short-row kernel on their
    compacted CSR -- instead of ``variant``."""
    dev = require_device(rowptr, col, alpha, V)
    code = _dtype_code(V, "pma_fwd")
    es = V.element_size()
    _f32(alpha, "pma_fwd logits")
    V = _rowmajor(V)
    if alpha.dim() != 2 or (alpha.shape[1] > 1 and alpha.stride(1) != 1) or 0 < split:
        alpha = alpha.contiguous()           # (a row-strided view is fine: the logits may sit beside the V rows)
    n_s, d = V.shape
    if d % heads != 0 or alpha.shape != (n_s, heads):
        raise _lib.AllSetHipError(f"pma_fwd: V {tuple(V.shape)} / alpha {tuple(alpha.shape)} inconsistent with heads={heads}")
    out = torch.empty((n_t, d), dtype=V.dtype, device=dev)
    m = torch.empty((n_t, heads), dtype=torch.float32, device=dev)
    l = torch.empty((n_t, heads), dtype=torch.float32, device=dev)
    algo = col.numel() * (es * d + 4 + 4 * heads) + (n_t + 1) * 4 + n_t * (d * es + 8 * heads)
    with on_device(dev), _timed("pma_fwd", dev, algo):
        if row_order is not None and row_order.numel() != n_t:
            row_order = None
        lib = _lib.load()
        if 0 < split < n_t and rowptr.numel() == n_t + 1:      # see segreduce: regular rows / singleton tail
            check(lib.allset_pma_fwd_ex(code, 1, col.numel(), None, ptr(rowptr), ptr(col), ptr(alpha), ptr(V), _ld(V), slope,
                                        ptr(out), max(d, 1), ptr(m), ptr(l), split, n_s, heads, d // heads, stream_of(dev)),
                  "allset_pma_fwd_ex")
            check(lib.allset_pma_fwd_ex(code, 2, col.numel(), None, ptr(rowptr[split:]), ptr(col), ptr(alpha), ptr(V), _ld(V), slope,
                                        ptr(out[split:]), max(d, 1), ptr(m[split:]), ptr(l[split:]), n_t - split, n_s, heads,
                                        d // heads, stream_of(dev)), "allset_pma_fwd_ex")
        elif sizes is not None and rowptr.numel() == n_t + 1:
            lda = alpha.stride(0) if n_s > 1 else heads
            check(lib.allset_pma_fwd_ld(code, 1, col.numel(), ptr(sizes.long_ids), ptr(rowptr), ptr(col), ptr(alpha), lda, ptr(V),
                                        _ld(V), slope, ptr(out), max(d, 1), ptr(m), ptr(l), sizes.long_ids.numel(), n_s, heads,
                                        d // heads, stream_of(dev)), "allset_pma_fwd_ld")
            check(lib.allset_pma_fwd_ld(code, 2, sizes.col_short.numel(), ptr(sizes.short_ids), ptr(sizes.rowptr_short),
                                        ptr(sizes.col_short), ptr(alpha), lda, ptr(V), _ld(V), slope, ptr(out), max(d, 1), ptr(m),
                                        ptr(l), sizes.short_ids.numel(), n_s, heads, d // heads, stream_of(dev)), "allset_pma_fwd_ld")
        else:
            lda = alpha.stride(0) if n_s > 1 else heads
            if variant == 2:
                row_order = None             # (the short-row kernel reads a row list as the ids of a COMPACTED CSR: see ``sizes``)
            check(lib.allset_pma_fwd_ld(code, variant, col.numel(), ptr(row_order), ptr(rowptr), ptr(col), ptr(alpha), lda, ptr(V),
                                        _ld(V), slope, ptr(out), max(d, 1), ptr(m), ptr(l), n_t, n_s, heads, d // heads,
                                        stream_of(dev)), "allset_pma_fwd_ld")
    return out, m, l


def pma_attention(rowptr: Tensor, col: Tensor, alpha: Tensor, m: Tensor, l: Tensor, slope: float) -> Tensor:
    dev = require_device(rowptr, col, alpha, m, l)
    n_t, heads = m.shape
    p = torch.empty((col.numel(), heads), dtype=torch.float32, device=dev)
    with on_device(dev):
        check(_lib.load().allset_pma_attention(ptr(rowptr), ptr(col), ptr(alpha.contiguous()), ptr(m), ptr(l), slope,
                                               ptr(p), n_t, heads, stream_of(dev)), "allset_pma_attention")
    return p


def pma_bwd_stats(out: Tensor, gout: Tensor, m: Tensor, l: Tensor, stats: Optional[Tensor] = None) -> Tensor:
    """``stats`` (optional): a float32 [n_t, H, 2] destination, possibly a row-strided view (e.g. beside a copy of the
    ``gout`` rows, see ``pma_bwd_src``)."""
    dev = require_device(out, gout, m, l)
    code = _dtype_code(out, "pma_bwd_stats")
    if gout.dtype != out.dtype:
        gout = gout.to(out.dtype)
    es = out.element_size()
    out, gout = _rowmajor(out), _rowmajor(gout)
    n_t, d = out.shape
    heads = m.shape[1]
    if stats is None:
        stats = torch.empty((n_t, heads, 2), dtype=torch.float32, device=dev)
    elif stats.shape != (n_t, heads, 2) or stats.dtype != torch.float32 or stats.stride(2) != 1 or stats.stride(1) != 2:
        raise _lib.AllSetHipError("pma_bwd_stats: stats must be float32 [n_t, H, 2] with contiguous rows")
    lds = stats.stride(0) if n_t > 1 else 2 * heads
    algo = n_t * (2 * d * es + 8 * heads + 8 * heads)
    with on_device(dev), _timed("pma_bwd_stats", dev, algo):
        check(_lib.load().allset_pma_bwd_stats_ld(code, ptr(out), _ld(out), ptr(gout), _ld(gout), ptr(m.contiguous()),
                                                  ptr(l.contiguous()), ptr(stats), lds, n_t, heads, d // heads, stream_of(dev)),
              "allset_pma_bwd_stats_ld")
    return stats


def pma_bwd_src(rowptrT: Tensor, colT: Tensor, alpha: Tensor, V: Tensor, gout: Tensor, stats: Tensor, slope: float,
                variant: int = 0, row_order: Optional[Tensor] = None, split: int = -1, sizes: Optional[SizeSplit] = None
                ) -> Tuple[Tensor, Tensor]:
    dev = require_device(rowptrT, colT, alpha, V, gout, stats)
    code = _dtype_code(V, "pma_bwd_src")
    if gout.dtype != V.dtype:
        gout = gout.to(V.dtype)
    es = V.element_size()
    _f32(alpha, "pma_bwd_src logits")
    V, gout = _rowmajor(V), _rowmajor(gout)
    alpha = alpha.contiguous()
    n_s, d = V.shape
    n_t = gout.shape[0]
    heads = alpha.shape[1]
    gV = torch.empty((n_s, d), dtype=V.dtype, device=dev)
    galpha = torch.empty((n_s, heads), dtype=torch.float32, device=dev)
    stats = stats.view(n_t, heads, 2) if stats.is_contiguous() else stats
    if (stats.dim() != 3 or stats.stride(2) != 1 or stats.stride(1) != 2 or 0 < split < n_s):
        stats = stats.contiguous().view(n_t, heads, 2)           # (a row-strided view is fine: stats may sit beside gout rows)
    lds = stats.stride(0) if n_t > 1 else 2 * heads
    algo = colT.numel() * (es * d + 4 + 8 * heads) + (n_s + 1) * 4 + n_s * (2 * d * es + 8 * heads)
    with on_device(dev), _timed("pma_bwd_src", dev, algo):
        if row_order is not None and row_order.numel() != n_s:
            row_order = None
        lib = _lib.load()
        if 0 < split < n_s and rowptrT.numel() == n_s + 1:     # rows of this CSR are the SOURCES (alpha / V / gV rows)
            check(lib.allset_pma_bwd_src_ex(code, 1, colT.numel(), None, ptr(rowptrT), ptr(colT), ptr(alpha), ptr(V), _ld(V),
                                            ptr(gout), _ld(gout), ptr(stats), slope, ptr(gV), max(d, 1), ptr(galpha), split, n_t,
                                            heads, d // heads, stream_of(dev)), "allset_pma_bwd_src_ex")
            check(lib.allset_pma_bwd_src_ex(code, 2, colT.numel(), None, ptr(rowptrT[split:]), ptr(colT), ptr(alpha[split:]),
                                            ptr(V[split:]), _ld(V), ptr(gout), _ld(gout), ptr(stats), slope, ptr(gV[split:]),
                                            max(d, 1), ptr(galpha[split:]), n_s - split, n_t, heads, d // heads, stream_of(dev)),
                  "allset_pma_bwd_src_ex")
        elif sizes is not None and rowptrT.numel() == n_s + 1:
            check(lib.allset_pma_bwd_src_ld(code, 1, colT.numel(), ptr(sizes.long_ids), ptr(rowptrT), ptr(colT), ptr(alpha), ptr(V),
                                            _ld(V), ptr(gout), _ld(gout), ptr(stats), lds, slope, ptr(gV), max(d, 1),
                                            ptr(galpha), sizes.long_ids.numel(), n_t, heads, d // heads, stream_of(dev)),
                  "allset_pma_bwd_src_ld")
            check(lib.allset_pma_bwd_src_ld(code, 2, sizes.col_short.numel(), ptr(sizes.short_ids), ptr(sizes.rowptr_short),
                                            ptr(sizes.col_short), ptr(alpha), ptr(V), _ld(V), ptr(gout), _ld(gout), ptr(stats), lds,
                                            slope, ptr(gV), max(d, 1), ptr(galpha), sizes.short_ids.numel(), n_t, heads, d // heads,
                                            stream_of(dev)), "allset_pma_bwd_src_ld")
        else:
            if variant == 2:
                row_order = None
            check(lib.allset_pma_bwd_src_ld(code, variant, colT.numel(), ptr(row_order), ptr(rowptrT), ptr(colT), ptr(alpha), ptr(V),
                                            _ld(V), ptr(gout), _ld(gout), ptr(stats), lds, slope, ptr(gV), max(d, 1),
                                            ptr(galpha), n_s, n_t, heads, d // heads, stream_of(dev)),
                  "allset_pma_bwd_src_ld")
    return gV, galpha


def block_transpose(x: Tensor, world: int, to_blocks: bool) -> Tensor:
    """The pack / unpack copy of the column-sharded layer's all-to-all.  ``to_blocks``: [rows, P*dc] row-major ->
    [P, rows, dc]; else [P, rows, dc] -> [rows, P*dc].  Needs dc * element_size to be a multiple of 16."""
    dev = require_device(x)
    es = x.element_size()
    if to_blocks:
        x = _rowmajor(x)
        rows, d = x.shape
        dc = d // world
        out = torch.empty((world, rows, dc), dtype=x.dtype, device=dev)
        ld = _ld(x) * es
    else:
        x = x.contiguous()
        _, rows, dc = x.shape
        out = torch.empty((rows, world * dc), dtype=x.dtype, device=dev)
        ld = world * dc * es
    with on_device(dev), _timed("block_transpose", dev, 2 * rows * world * dc * es):
        check(_lib.load().allset_block_transpose(ptr(x), ptr(out), rows, world, dc * es, ld, int(to_blocks), stream_of(dev)),
              "allset_block_transpose")
    return out


def block_transpose_supported(x: Tensor, world: int, to_blocks: bool) -> bool:
    if not x.is_cuda:
        return False
    dc = (x.shape[1] // world) if to_blocks else x.shape[2]
    return (dc * x.element_size()) % 16 == 0 and dc > 0 and (not to_blocks or x.shape[1] % world == 0)


def pma_merge_pack(out_loc: Tensor, m_loc: Tensor, l_loc: Tensor, m_glob: Tensor, heads: int) -> Tensor:
    """[n, d + H] rows ``[out_loc * w | w]`` with ``w = l_loc * exp(m_loc - m_glob)`` (0 where ``l_loc == 0``): this rank's
    numerators / denominators relative to the global row maximum, ready for a sum-reduce-scatter."""
    dev = require_device(out_loc, m_loc, l_loc, m_glob)
    _f32(out_loc, "pma_merge_pack")
    out_loc = _rowmajor(out_loc)
    n, d = out_loc.shape
    width = d + heads
    ldp = (width + 3) // 4 * 4
    buf = torch.empty((n, ldp), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("pma_merge_pack", dev, n * (2 * d + 4 * heads) * 4):
        check(_lib.load().allset_pma_merge_pack(ptr(out_loc), _ld(out_loc), ptr(m_loc.contiguous()), ptr(l_loc.contiguous()),
                                                ptr(m_glob.contiguous()), ptr(buf), ldp, n, heads, d // heads, stream_of(dev)),
              "allset_pma_merge_pack")
    return buf if ldp == width else buf[:, :width]


# ---- degree-scaled propagate of the hypergraph-convolution baselines (csrc/hconv.hip) -----------------------------------------
# activation codes of the row epilogue (csrc/row_epilogue.h): the hops built with the elu branch (hconv, hattn), and the relu-only ones
HCONV_ACTS = {None: _lib.ACT_NONE, "none": _lib.ACT_NONE, "relu": _lib.ACT_RELU, "elu": _lib.ACT_ELU}
RELU_ACTS = {k: v for k, v in HCONV_ACTS.items() if k != "elu"}


def _hconv_variant(csr: CSR, n_t: int, flat_ok: bool, variant: Optional[int]) -> int:
    """None: the CSR's own choice (the short-row kernel only where it is built).  1 / 2 go to the C entry as given, which refuses
    a 2 the short-row kernel cannot take."""
    if variant is None:
        return csr.variant("segreduce", n_t) if flat_ok else 1
    if variant not in (1, 2):
        raise _lib.AllSetHipError(f"hconv_propagate: variant must be None, 1 or 2, got {variant!r}")
    return int(variant)


def hconv_propagate(csr: CSR, x: Tensor, n_t: int, r: Optional[Tensor] = None, s: Optional[Tensor] = None,
                    bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0, seed: int = 0,
                    seed_base: Optional[Tensor] = None, variant: Optional[int] = None) -> Tensor:
    """``y[t] = drop_p(act(s[t] * sum_{j in row t} r[col_j] * x[col_j] + bias))`` over ``csr`` (rows = outputs, the first ``n_t``
    rows of it).  ``r`` f32[n_s], ``s`` f32[n_t], ``bias`` f32[d]: each optional.  fp32 only.  ``variant``: kernel variant override
    (tests): 1 one wavefront per row, 2 the short-row kernel (16-byte rows of width <= 256 only, anything else raises); None = the
    CSR's own choice."""
    dev = require_device(csr.rowptr, x, r, s, bias)
    _f32(x, "hconv_propagate")
    for t, what in ((r, "r"), (s, "s"), (bias, "bias")):
        if t is not None:
            _f32(t, f"hconv_propagate {what}")
    r = r.contiguous() if r is not None else None
    s = s.contiguous() if s is not None else None
    bias = bias.contiguous() if bias is not None else None
    x = _rowmajor(x)
    n_s, d = x.shape
    if r is not None and r.numel() < n_s:
        raise _lib.AllSetHipError(f"hconv_propagate: r has {r.numel()} entries for {n_s} gathered rows")
    if s is not None and s.numel() < n_t:
        raise _lib.AllSetHipError(f"hconv_propagate: s has {s.numel()} entries for {n_t} output rows")
    if bias is not None and bias.numel() != d:
        raise _lib.AllSetHipError(f"hconv_propagate: bias has {bias.numel()} entries for width {d}")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"hconv_propagate: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    y = torch.empty((n_t, d), dtype=torch.float32, device=dev)
    nnz = csr.col.numel()
    flat_ok = d % 4 == 0 and d <= 256 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
    variant = _hconv_variant(csr, n_t, flat_ok, variant)
    order = csr.row_order if (variant == 1 and csr.row_order is not None and csr.row_order.numel() == n_t) else None
    algo = nnz * (4 * d + 4 + (4 if r is not None else 0)) + (n_t + 1) * 4 + n_t * 4 * d
    with on_device(dev), _timed("hconv_fwd", dev, algo):
        check(_lib.load().allset_hconv_fwd(variant, nnz, ptr(order), ptr(csr.rowptr), ptr(csr.col), ptr(r), ptr(s), ptr(x), _ld(x),
                                           ptr(bias), HCONV_ACTS[act], float(p), int(seed), ptr(seed_base), ptr(y), max(d, 1),
                                           n_t, n_s, d, stream_of(dev)), "allset_hconv_fwd")
    return y


def hconv_propagate_w(csr: CSR, x: Tensor, n_t: int, w: Optional[Tensor] = None, bias: Optional[Tensor] = None,
                      act: Optional[str] = None, p: float = 0.0, seed: int = 0, seed_base: Optional[Tensor] = None,
                      variant: Optional[int] = None) -> Tensor:
    """``y[t] = drop_p(act(sum_{j in row t} w[j] * x[col_j] + bias))`` over ``csr`` with ``w`` f32[nnz] per incidence in ``csr``'s
    own order (None = ones).  fp32 only.  ``variant``: as :func:`hconv_propagate`'s."""
    dev = require_device(csr.rowptr, x, w, bias)
    _f32(x, "hconv_propagate_w")
    for t, what in ((w, "w"), (bias, "bias")):
        if t is not None:
            _f32(t, f"hconv_propagate_w {what}")
    w = w.contiguous() if w is not None else None
    bias = bias.contiguous() if bias is not None else None
    x = _rowmajor(x)
    n_s, d = x.shape
    nnz = csr.col.numel()
    if w is not None and w.numel() != nnz:
        raise _lib.AllSetHipError(f"hconv_propagate_w: w has {w.numel()} entries for {nnz} incidences")
    if bias is not None and bias.numel() != d:
        raise _lib.AllSetHipError(f"hconv_propagate_w: bias has {bias.numel()} entries for width {d}")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"hconv_propagate_w: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    y = torch.empty((n_t, d), dtype=torch.float32, device=dev)
    flat_ok = d % 4 == 0 and d <= 256 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
    variant = _hconv_variant(csr, n_t, flat_ok, variant)
    order = csr.row_order if (variant == 1 and csr.row_order is not None and csr.row_order.numel() == n_t) else None
    algo = nnz * (4 * d + 4 + (4 if w is not None else 0)) + (n_t + 1) * 4 + n_t * 4 * d
    with on_device(dev), _timed("hconv_fwd_w", dev, algo):
        check(_lib.load().allset_hconv_fwd_w(variant, nnz, ptr(order), ptr(csr.rowptr), ptr(csr.col), ptr(w), None, ptr(x), _ld(x),
                                             ptr(bias), HCONV_ACTS[act], float(p), int(seed), ptr(seed_base), ptr(y), max(d, 1),
                                             n_t, n_s, d, stream_of(dev)), "allset_hconv_fwd_w")
    return y


# ---- clique expansion and its GCN normalisation (csrc/clique.hip) -----------------------------------------------------------------
def clique_pairs(rowptr: Tensor, member: Tensor, edge_of: Tensor) -> Tensor:
    """Every pair (member[a], member[b]), a < b, of every row of the hyperedge -> member CSR (``rowptr`` int32[n_e + 1], ``member``
    int32 ascending within rows, ``edge_of`` int32 the row of each position) as int64 keys ``member[a] << 32 | member[b]``, rows in
    order.  Raises ``ValueError`` before emitting when the pair count would not fit an int32-indexed CSR."""
    dev = require_device(rowptr, member, edge_of)
    n_e, nnz = rowptr.numel() - 1, member.numel()
    lib = _lib.load()
    cnt = torch.empty(n_e, dtype=torch.int64, device=dev)
    with on_device(dev), _timed("clique_count", dev, (n_e + 1) * 4 + n_e * 8):
        check(lib.allset_clique_count(ptr(rowptr), n_e, ptr(cnt), stream_of(dev)), "allset_clique_count")
    off = torch.cumsum(cnt, 0) - cnt
    total = int(cnt.sum()) if n_e > 0 else 0                                   # one host sync: the output size
    if total + nnz >= 2 ** 31 - 1:
        raise ValueError(f"clique expansion: {total} vertex pairs do not fit an int32-indexed CSR (at most {2 ** 31 - 2 - nnz} here)")
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    with on_device(dev), _timed("clique_emit", dev, nnz * 16 + n_e * 8 + total * 12):
        check(lib.allset_clique_emit(ptr(rowptr), ptr(member), ptr(edge_of), ptr(off), nnz, ptr(keys), stream_of(dev)),
              "allset_clique_emit")
    return keys


def spgemm_bool_bins() -> Tuple[int, int, int, int]:
    """The boolean product's row bins: ``(hash16 candidates, hash64 candidates, bitmap window columns, entries of an A row from which
    every thread walks its own)`` -- see include/allset_hip_ext.h."""
    out = (c_int64_t * 4)()
    check(_lib.load().allset_spgemm_bool_bins(out), "allset_spgemm_bool_bins")
    return tuple(int(v) for v in out)


def spgemm_bool(rowptr_a: Tensor, col_a: Tensor, rowptr_b: Tensor, col_b: Tensor, n_c: int,
                workspace: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """``pattern(A B)`` of two int32 device CSRs (``A`` [n_a, n_b], ``B`` [n_b, n_c]; duplicates count once) as int32 CSR ``(rowptr
    [n_a + 1], col [nnz_c])`` with strictly increasing columns in every row: count pass, scan, fill pass (csrc/metapath.hip).  Device
    memory: the result, 8 bytes per row of ``A`` for the scan, and the workspace (``workspace``: a uint8 device tensor of at least
    ``allset_spgemm_bool_workspace_bytes(n_a)`` bytes, allocated here when None) -- nothing grows with the candidate count.  One
    host sync: the result's size."""
    dev = require_device(rowptr_a, col_a, rowptr_b, col_b, workspace)
    for t, what in ((rowptr_a, "rowptr_a"), (col_a, "col_a"), (rowptr_b, "rowptr_b"), (col_b, "col_b")):
        if t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous():
            raise _lib.AllSetHipError(f"spgemm_bool: {what} must be a contiguous int32 vector (got {t.dtype} {tuple(t.shape)})")
    n_a, n_b = rowptr_a.numel() - 1, rowptr_b.numel() - 1
    if n_a < 0 or n_b < 0:
        raise _lib.AllSetHipError("spgemm_bool: an empty rowptr (a CSR of n rows has n + 1 entries)")
    lib = _lib.load()
    need = c_size_t(0)
    check(lib.allset_spgemm_bool_workspace_bytes(n_a, byref(need)), "allset_spgemm_bool_workspace_bytes")
    if workspace is None:
        workspace = torch.empty(max(need.value, 1), dtype=torch.uint8, device=dev)
    elif workspace.dtype != torch.uint8 or not workspace.is_contiguous():
        raise _lib.AllSetHipError("spgemm_bool: workspace must be a contiguous uint8 tensor")
    ws_bytes = workspace.numel()
    cnt = torch.empty(n_a, dtype=torch.int32, device=dev)
    nnz_a, nnz_b = col_a.numel(), col_b.numel()
    with on_device(dev), _timed("spgemm_bool_count", dev, (n_a + n_b) * 4 + nnz_a * 4 + n_a * 4):
        check(lib.allset_spgemm_bool_count(ptr(rowptr_a), ptr(col_a), ptr(rowptr_b), ptr(col_b), n_a, n_b, int(n_c), ptr(cnt),
                                           ptr(workspace), ws_bytes, stream_of(dev)), "allset_spgemm_bool_count")
    rowptr64 = torch.zeros(n_a + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, dtype=torch.int64, out=rowptr64[1:])
    nnz_c = int(rowptr64[-1])                                                  # one host sync: the output size
    col = torch.empty(nnz_c if nnz_c <= 2 ** 31 - 1 else 0, dtype=torch.int32, device=dev)
    rowptr = rowptr64.clamp_(max=2 ** 31 - 1).to(torch.int32)                  # (beyond int32 the fill refuses before reading it)
    with on_device(dev), _timed("spgemm_bool_fill", dev, (n_a + n_b) * 4 + nnz_a * 4 + n_a * 4 + nnz_c * 4):
        check(lib.allset_spgemm_bool_fill(ptr(rowptr_a), ptr(col_a), ptr(rowptr_b), ptr(col_b), n_a, n_b, int(n_c), ptr(rowptr), nnz_c,
                                          ptr(col), ptr(workspace), ws_bytes, stream_of(dev)), "allset_spgemm_bool_fill")
    return rowptr, col


# ---- leave-one-out segmented sums: exclude-self aggregation without the expanded edge list (csrc/loo.hip) -------------------------
def loo_supported(d: int) -> bool:
    return bool(_lib.load().allset_loo_supported(int(d)))


def loo_long_threshold() -> int:
    """Segments longer than this are summed by a workgroup each (``long_seg`` of :func:`loo_rows` lists them)."""
    return int(_lib.load().allset_loo_long_threshold())


def loo_rows(rowptr: Tensor, col: Optional[Tensor], src: Tensor, s_src: Optional[Tensor] = None, s_seg: Optional[Tensor] = None,
             long_seg: Optional[Tensor] = None, n_long: Optional[int] = None) -> Tensor:
    """``out[p] = s_seg[g] * sum_{q in segment g, q != p} s_src[idx(q)] * src[idx(q)]`` for every position ``p`` of the CSR ``rowptr``
    (int32[n_seg + 1]); a segment of one position keeps its own row.  ``idx(q) = col[q]`` (int32[nnz]), or ``q`` itself with
    ``col=None`` (``src`` holds the nnz rows).  ``s_src`` f32[src rows] and ``s_seg`` f32[n_seg] are optional.  ``long_seg``: int32 ids
    of the segments longer than :func:`loo_long_threshold` (``None``: each segment's length is looked at on the device); ``n_long=0``
    with ``long_seg=None`` states there is none.  Returns f32 [nnz, d].  fp32 only, d % 4 == 0, d <= 512: anything else raises."""
    dev = require_device(rowptr, col, src, s_src, s_seg, long_seg)
    if src.dtype != torch.float32:
        raise NotImplementedError(f"loo_rows: float32 only (got {src.dtype}); bf16 storage keeps the expansion path "
                                  "(preprocessing.expand_edge_index)")
    for t, what in ((rowptr, "rowptr"), (col, "col"), (long_seg, "long_seg")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
            raise _lib.AllSetHipError(f"loo_rows: {what} must be a contiguous int32 vector (got {t.dtype} {tuple(t.shape)})")
    for t, what in ((s_src, "s_src"), (s_seg, "s_seg")):
        if t is not None:
            _f32(t, f"loo_rows {what}")
            if t.dim() != 1 or not t.is_contiguous():
                raise _lib.AllSetHipError(f"loo_rows: {what} must be a contiguous vector")
    src = _rowmajor(src)
    n_src, d = src.shape
    n_seg = rowptr.numel() - 1
    if n_seg < 0:
        raise _lib.AllSetHipError("loo_rows: an empty rowptr (a CSR of n segments has n + 1 entries)")
    nnz = int(col.numel()) if col is not None else n_src
    if s_src is not None and s_src.numel() < n_src:
        raise _lib.AllSetHipError(f"loo_rows: s_src has {s_src.numel()} entries for {n_src} source rows")
    if s_seg is not None and s_seg.numel() < n_seg:
        raise _lib.AllSetHipError(f"loo_rows: s_seg has {s_seg.numel()} entries for {n_seg} segments")
    if d > 0 and not loo_supported(d):
        raise _lib.AllSetHipError(f"loo_rows: width {d} is not built (d % 4 == 0, d <= 512); there is no fallback")
    if src.stride(0) % 4 != 0 or src.data_ptr() % 16 != 0:
        src = src.contiguous()
    if long_seg is not None:
        n_long = int(long_seg.numel())
    elif n_long is None:
        n_long = -1
    elif n_long != 0:
        raise _lib.AllSetHipError("loo_rows: n_long without long_seg can only state 0")
    out = torch.empty((nnz, d), dtype=torch.float32, device=dev)
    algo = nnz * (2 * d * 4 + (4 if col is not None else 0) + (4 if s_src is not None else 0)) + (n_seg + 1) * 4
    with on_device(dev), _timed("loo_rows", dev, algo):
        check(_lib.load().allset_loo_rows(ptr(rowptr), ptr(col), ptr(src), _ld(src), ptr(s_src), ptr(s_seg), ptr(out), max(d, 1),
                                          ptr(long_seg) if n_long > 0 else None, n_long, n_seg, n_src, nnz, d, stream_of(dev)),
              "allset_loo_rows")
    return out


# ---- CEGCN's GCN hop without the clique expansion: segmented exclusive scan + per-vertex collect (csrc/scan.hip) --------------------
def scan_rows_supported(d: int) -> bool:
    return bool(_lib.load().allset_scan_rows_supported(int(d)))


def scan_rows(rowptr: Tensor, col: Optional[Tensor], src: Tensor, s_src: Optional[Tensor] = None, reverse: bool = False,
              long_seg: Optional[Tensor] = None, n_long: Optional[int] = None) -> Tensor:
    """``out[p] = sum_{q in p's segment, q before p (reverse: behind p)} s_src[idx(q)] * src[idx(q)]`` for every position ``p`` of the CSR
    ``rowptr`` (int32[n_seg + 1]): an exclusive prefix (suffix) sum per segment, zeros where there is nothing in front (behind).
    ``idx(q) = col[q]`` (int32[nnz]), or ``q`` itself with ``col=None``.  ``s_src`` f32[src rows] is optional.  ``long_seg`` /
    ``n_long``: as for :func:`loo_rows` (the same threshold).  Returns f32 [nnz, d].  fp32 only, d % 4 == 0, d <= 512: anything else
    raises."""
    dev = require_device(rowptr, col, src, s_src, long_seg)
    if src.dtype != torch.float32:
        raise NotImplementedError(f"scan_rows: float32 only (got {src.dtype}); bf16 storage is not built")
    for t, what in ((rowptr, "rowptr"), (col, "col"), (long_seg, "long_seg")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
            raise _lib.AllSetHipError(f"scan_rows: {what} must be a contiguous int32 vector (got {t.dtype} {tuple(t.shape)})")
    if s_src is not None:
        _f32(s_src, "scan_rows s_src")
        if s_src.dim() != 1 or not s_src.is_contiguous():
            raise _lib.AllSetHipError("scan_rows: s_src must be a contiguous vector")
    src = _rowmajor(src)
    n_src, d = src.shape
    n_seg = rowptr.numel() - 1
    if n_seg < 0:
        raise _lib.AllSetHipError("scan_rows: an empty rowptr (a CSR of n segments has n + 1 entries)")
    nnz = int(col.numel()) if col is not None else n_src
    if s_src is not None and s_src.numel() < n_src:
        raise _lib.AllSetHipError(f"scan_rows: s_src has {s_src.numel()} entries for {n_src} source rows")
    if d > 0 and not scan_rows_supported(d):
        raise _lib.AllSetHipError(f"scan_rows: width {d} is not built (d % 4 == 0, d <= 512); there is no fallback")
    if src.stride(0) % 4 != 0 or src.data_ptr() % 16 != 0:
        src = src.contiguous()
    if long_seg is not None:
        n_long = int(long_seg.numel())
    elif n_long is None:
        n_long = -1
    elif n_long != 0:
        raise _lib.AllSetHipError("scan_rows: n_long without long_seg can only state 0")
    out = torch.empty((nnz, d), dtype=torch.float32, device=dev)
    algo = nnz * (2 * d * 4 + (4 if col is not None else 0) + (4 if s_src is not None else 0)) + (n_seg + 1) * 4
    with on_device(dev), _timed("scan_rows", dev, algo):
        check(_lib.load().allset_scan_rows(ptr(rowptr), ptr(col), ptr(src), _ld(src), ptr(s_src), ptr(out), max(d, 1),
                                           ptr(long_seg) if n_long > 0 else None, n_long, int(bool(reverse)), n_seg, n_src, nnz, d,
                                           stream_of(dev)), "allset_scan_rows")
    return out


def scan_collect(rowptr: Tensor, col: Tensor, t: Tensor, x: Optional[Tensor] = None, r_self: Optional[Tensor] = None,
                 s: Optional[Tensor] = None, bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0, seed: int = 0,
                 seed_base: Optional[Tensor] = None, width: Optional[int] = None) -> Tensor:
    """``y[j] = drop_p(act(s[j] * (sum_{q in row j} t[col[q]] + r_self[j] * x[j]) + bias))`` over the CSR ``rowptr`` (int32[n + 1]) /
    ``col`` (int32, rows of ``t``).  ``r_self`` / ``s`` f32[n] and ``bias`` f32[width] are optional.  ``width`` (default d): the columns
    that carry the epilogue -- the dropout mask is that of an [n, width] matrix -- the d - width < 4 columns behind them are written
    as zeros.  Returns f32 [n, d].  fp32 only, d % 4 == 0, d <= 512: anything else raises."""
    dev = require_device(rowptr, col, t, x, r_self, s, bias)
    _f32(t, "scan_collect")
    for v, what in ((x, "x"), (r_self, "r_self"), (s, "s"), (bias, "bias")):
        if v is not None:
            _f32(v, f"scan_collect {what}")
    for v, what in ((rowptr, "rowptr"), (col, "col")):
        if v.dtype != torch.int32 or v.dim() != 1 or not v.is_contiguous():
            raise _lib.AllSetHipError(f"scan_collect: {what} must be a contiguous int32 vector (got {v.dtype} {tuple(v.shape)})")
    t = _rowmajor(t)
    n_pos, d = t.shape
    n = rowptr.numel() - 1
    width = d if width is None else int(width)
    if n < 0:
        raise _lib.AllSetHipError("scan_collect: an empty rowptr (a CSR of n rows has n + 1 entries)")
    if d > 0 and not scan_rows_supported(d):
        raise _lib.AllSetHipError(f"scan_collect: width {d} is not built (d % 4 == 0, d <= 512); there is no fallback")
    if (r_self is None) != (x is None):
        raise _lib.AllSetHipError("scan_collect: give x and r_self together, or neither")
    if x is not None:
        x = _rowmajor(x)
        if tuple(x.shape) != (n, d):
            raise _lib.AllSetHipError(f"scan_collect: x is {tuple(x.shape)}, expected ({n}, {d})")
        if x.stride(0) % 4 != 0 or x.data_ptr() % 16 != 0:
            x = x.contiguous()
    for v, what in ((r_self, "r_self"), (s, "s")):
        if v is not None and (v.dim() != 1 or not v.is_contiguous() or v.numel() < n):
            raise _lib.AllSetHipError(f"scan_collect: {what} must be a contiguous vector of at least {n} entries")
    if bias is not None and (not bias.is_contiguous() or bias.numel() != width):
        raise _lib.AllSetHipError(f"scan_collect: bias has {bias.numel()} entries for width {width}")
    if t.stride(0) % 4 != 0 or t.data_ptr() % 16 != 0:
        t = t.contiguous()
    y = torch.empty((n, d), dtype=torch.float32, device=dev)
    algo = col.numel() * (4 * d + 4) + (n + 1) * 4 + n * (4 * d + (4 * d + 4 if x is not None else 0) + (4 if s is not None else 0))
    with on_device(dev), _timed("scan_collect", dev, algo):
        check(_lib.load().allset_scan_collect(ptr(rowptr), ptr(col), ptr(t), _ld(t), ptr(r_self), ptr(x), _ld(x) if x is not None else 0,
                                              ptr(s), ptr(bias), HCONV_ACTS[act], float(p), int(seed), ptr(seed_base), ptr(y),
                                              max(d, 1), n, n_pos, d, width, stream_of(dev)), "allset_scan_collect")
    return y


# ---- leave-one-out softmax: the exclude-self PMA pooling without the expanded edge list (csrc/loo_softmax.hip) --------------------
def loo_softmax_supported(d: int, heads: int) -> bool:
    return bool(_lib.load().allset_loo_softmax_supported(int(d), int(heads)))


def _loo_softmax_args(who: str, rowptr: Tensor, col: Optional[Tensor], alpha: Tensor, V: Tensor, heads: int, long_seg: Optional[Tensor],
                      n_long: Optional[int], extra: Tuple[Optional[Tensor], ...] = ()):
    """The checks both passes share; returns (device, V row-major and aligned, n_seg, n_src, nnz, d, n_long)."""
    dev = require_device(rowptr, col, alpha, V, long_seg, *extra)
    if V.dtype != torch.float32 or alpha.dtype != torch.float32:
        raise NotImplementedError(f"{who}: float32 only (got V {V.dtype}, alpha {alpha.dtype}); bf16 storage keeps the expansion path "
                                  "(preprocessing.expand_edge_index)")
    for t, what in ((rowptr, "rowptr"), (col, "col"), (long_seg, "long_seg")):
        if t is not None and (t.dtype != torch.int32 or t.dim() != 1 or not t.is_contiguous()):
            raise _lib.AllSetHipError(f"{who}: {what} must be a contiguous int32 vector (got {t.dtype} {tuple(t.shape)})")
    V = _rowmajor(V)
    n_src, d = V.shape
    heads = int(heads)
    n_seg = rowptr.numel() - 1
    if n_seg < 0:
        raise _lib.AllSetHipError(f"{who}: an empty rowptr (a CSR of n segments has n + 1 entries)")
    if heads < 1 or alpha.dim() != 2 or tuple(alpha.shape) != (n_src, heads):
        raise _lib.AllSetHipError(f"{who}: alpha must be [{n_src}, {heads}] (one logit per source row and head), got {tuple(alpha.shape)}")
    if d > 0 and not loo_softmax_supported(d, heads):
        raise _lib.AllSetHipError(f"{who}: d = {d} with {heads} heads is not built (heads 1 | 2 | 4 | 8, (d / heads) % 4 == 0, d <= 512); "
                                  "there is no fallback")
    if V.stride(0) % 4 != 0 or V.data_ptr() % 16 != 0:
        V = V.contiguous()
    nnz = int(col.numel()) if col is not None else n_src
    if long_seg is not None:
        n_long = int(long_seg.numel())
    elif n_long is None:
        n_long = -1
    elif n_long != 0:
        raise _lib.AllSetHipError(f"{who}: n_long without long_seg can only state 0")
    return dev, V, n_seg, n_src, nnz, d, n_long


def loo_softmax_fwd(rowptr: Tensor, col: Optional[Tensor], alpha: Tensor, V: Tensor, heads: int, negative_slope: float = 0.2,
                    long_seg: Optional[Tensor] = None, n_long: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """Leave-one-out softmax pooling: for every position ``p`` of every segment of the CSR ``rowptr`` and every head ``h``, with
    ``a_q = leaky_relu(alpha[idx(q), h])``, ``out[p, h] = sum_{q != p} exp(a_q) V[idx(q), h] / Z_p`` and ``lse[p, h] = log Z_p``,
    ``Z_p = sum_{q != p} exp(a_q)``; a segment of one position keeps its row (``out = V[idx(p)]``, ``lse = a_p``).  ``idx(q) =
    col[q]``, or ``q`` itself with ``col=None``.  ``long_seg`` / ``n_long`` as for :func:`loo_rows`.  Returns ``(out f32[nnz, d], lse
    f32[nnz, heads])``.  fp32, heads 1 | 2 | 4 | 8, (d / heads) % 4 == 0, d <= 512: anything else raises."""
    dev, V, n_seg, n_src, nnz, d, n_long = _loo_softmax_args("loo_softmax_fwd", rowptr, col, alpha, V, heads, long_seg, n_long)
    alpha = alpha.contiguous()
    out = torch.empty((nnz, d), dtype=torch.float32, device=dev)
    lse = torch.empty((nnz, int(heads)), dtype=torch.float32, device=dev)
    algo = nnz * ((2 * d + 2 * int(heads)) * 4 + (4 if col is not None else 0)) + (n_seg + 1) * 4
    with on_device(dev), _timed("loo_softmax_fwd", dev, algo):
        check(_lib.load().allset_loo_softmax_fwd(ptr(rowptr), ptr(col), ptr(alpha), ptr(V), _ld(V), float(negative_slope), ptr(out),
                                                 max(d, 1), ptr(lse), ptr(long_seg) if n_long > 0 else None, n_long, n_seg, n_src, nnz,
                                                 d, int(heads), stream_of(dev)), "allset_loo_softmax_fwd")
    return out, lse


def loo_softmax_bwd(rowptr: Tensor, col: Optional[Tensor], alpha: Tensor, V: Tensor, heads: int, negative_slope: float, out: Tensor,
                    lse: Tensor, gout: Tensor, glse: Optional[Tensor] = None, long_seg: Optional[Tensor] = None,
                    n_long: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The backward of :func:`loo_softmax_fwd` PER POSITION: ``(gV_pos f32[nnz, d], galpha_pos f32[nnz, heads])``, the gradients that
    reach ``V[idx(q)]`` and ``alpha[idx(q)]`` through position ``q`` (with ``col`` the caller sums the positions of a source row).
    ``out`` / ``lse``: the forward's results; ``gout`` [nnz, d] and ``glse`` [nnz, heads] (``None``: zeros) their cotangents."""
    dev, V, n_seg, n_src, nnz, d, n_long = _loo_softmax_args("loo_softmax_bwd", rowptr, col, alpha, V, heads, long_seg, n_long,
                                                             (out, lse, gout, glse))
    H = int(heads)
    for t, what, shape in ((out, "out", (nnz, d)), (gout, "gout", (nnz, d)), (lse, "lse", (nnz, H)), (glse, "glse", (nnz, H))):
        if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != shape):
            raise _lib.AllSetHipError(f"loo_softmax_bwd: {what} must be float32 {shape}, got {t.dtype} {tuple(t.shape)}")
    alpha, out, gout, lse = alpha.contiguous(), out.contiguous(), gout.contiguous(), lse.contiguous()
    glse = glse.contiguous() if glse is not None else None
    gV = torch.empty((nnz, d), dtype=torch.float32, device=dev)
    galpha = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    scratch = torch.empty((nnz, H, 2), dtype=torch.float32, device=dev)          # parked suffix states of runs longer than a tile
    algo = nnz * ((4 * d + (4 if glse is not None else 3) * H) * 4 + (4 if col is not None else 0)) + (n_seg + 1) * 4
    with on_device(dev), _timed("loo_softmax_bwd", dev, algo):
        check(_lib.load().allset_loo_softmax_bwd(ptr(rowptr), ptr(col), ptr(alpha), ptr(V), _ld(V), float(negative_slope), ptr(out),
                                                 max(d, 1), ptr(lse), ptr(gout), max(d, 1), ptr(glse), ptr(gV), max(d, 1), ptr(galpha),
                                                 ptr(scratch), ptr(long_seg) if n_long > 0 else None, n_long, n_seg, n_src, nnz, d, H,
                                                 stream_of(dev)), "allset_loo_softmax_bwd")
    return gV, galpha


def gcn_norm(src: Tensor, dst: Tensor, m: Optional[Tensor], n: int) -> Tuple[Tensor, Tensor]:
    """torch_geometric 1.6.3 ``gcn_norm(edge_index, m, add_self_loops=True)`` for edges without self-loops, ids in [0, n):
    ``(edge_index int64[2, E + n] = [pairs | loops 0..n-1], w f32[E + n])``, ``w = deg^-1/2[src] * m * deg^-1/2[dst]``."""
    dev = require_device(src, dst, m)
    src, dst = src.contiguous(), dst.contiguous()
    if m is not None:
        _f32(m, "gcn_norm m")
        m = m.contiguous()
    E = src.numel()
    ei = torch.empty((2, E + n), dtype=torch.int64, device=dev)
    w = torch.empty(E + n, dtype=torch.float32, device=dev)
    deg = torch.empty(max(n, 1), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("gcn_norm", dev, E * (16 + 4 + 4) + (E + n) * (16 + 4) + n * 4):
        check(_lib.load().allset_gcn_norm(ptr(src), ptr(dst), ptr(m), E, n, ptr(deg), ptr(ei[0]), ptr(ei[1]), ptr(w), stream_of(dev)),
              "allset_gcn_norm")
    return ei, w


def hconv_bwd_epi(gy: Tensor, y: Tensor, act: Optional[str], p: float, seed: int, seed_base: Optional[Tensor],
                  want_bias: bool) -> Tuple[Tensor, Optional[Tensor]]:
    """Backward of :func:`hconv_propagate`'s epilogue: ``(g, part)`` with ``g = gy * keep / (1 - p) * act'(y)`` and, when
    ``want_bias``, the bias gradient's column partials [P, M] (M = d rounded up to 4) for ``dense.reduce_partials*``."""
    dev = require_device(gy, y)
    _f32(gy, "hconv_bwd_epi")
    gy, y = _rowmajor(gy), _rowmajor(y)
    n, d = y.shape
    g = torch.empty((n, d), dtype=torch.float32, device=dev)
    lib = _lib.load()
    part, P, M = None, 0, (d + 3) // 4 * 4
    if want_bias:
        ns = c_int64_t(0)
        check(lib.allset_hconv_bwd_epi_slices(n, byref(ns)), "allset_hconv_bwd_epi_slices")
        P = ns.value
        part = torch.empty((P, M), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("hconv_bwd_epi", dev, 3 * n * d * 4):
        check(lib.allset_hconv_bwd_epi(ptr(gy), _ld(gy), ptr(y), _ld(y), HCONV_ACTS[act], float(p), int(seed), ptr(seed_base),
                                       ptr(g), max(d, 1), ptr(part), P, M, n, d, stream_of(dev)), "allset_hconv_bwd_epi")
    return g, part


# ---- GAT attention hop of the clique-expansion baseline CEGAT (csrc/gat.hip) ----------------------------------------------------
GAT_MAX_HEADS, GAT_MAX_WIDTH = 64, 512


def _gat_order(csr: CSR, n_rows: int) -> Optional[Tensor]:
    return csr.row_order if (csr.row_order is not None and csr.row_order.numel() == n_rows) else None


def gat_fwd(csr: CSR, x: Tensor, al: Tensor, ar: Tensor, heads: int, slope: float, n_t: int, concat: bool = True,
            bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0, seed: int = 0,
            seed_base: Optional[Tensor] = None, want_grad: bool = False):
    """One GAT hop over ``csr`` (rows = targets, the first ``n_t`` of them): ``(y, agg, aggpos, ppos, m, l)``.  ``x`` f32[n_s, H*C],
    ``al`` f32[n_s, H], ``ar`` f32[n_t, H].  ``agg`` (the pre-epilogue rows) only in the head-mean form with ``want_grad``;
    ``aggpos`` / ``ppos`` (the positive-logit part of ``agg`` and of the softmax mass) only with ``want_grad``.  fp32 only."""
    dev = require_device(csr.rowptr, x, al, ar, bias)
    for t, what in ((x, "x"), (al, "al"), (ar, "ar"), (bias, "bias")):
        if t is not None:
            _f32(t, f"gat_fwd {what}")
    x, al, ar = _rowmajor(x), al.contiguous(), ar.contiguous()
    bias = bias.contiguous() if bias is not None else None
    n_s, d = x.shape
    H = int(heads)
    if H < 1 or d % H != 0 or d == 0:
        raise _lib.AllSetHipError(f"gat_fwd: width {d} does not split into {H} heads")
    C = d // H
    if tuple(al.shape) != (n_s, H) or tuple(ar.shape) != (n_t, H):
        raise _lib.AllSetHipError(f"gat_fwd: al {tuple(al.shape)} / ar {tuple(ar.shape)} against ({n_s}, {H}) / ({n_t}, {H})")
    width = d if concat else C
    if bias is not None and bias.numel() != width:
        raise _lib.AllSetHipError(f"gat_fwd: bias has {bias.numel()} entries for width {width}")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"gat_fwd: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    y = torch.empty((n_t, width), dtype=torch.float32, device=dev)
    m = torch.empty((n_t, H), dtype=torch.float32, device=dev)
    l = torch.empty((n_t, H), dtype=torch.float32, device=dev)
    agg = torch.empty((n_t, d), dtype=torch.float32, device=dev) if (want_grad and not concat) else None
    aggpos = torch.empty((n_t, d), dtype=torch.float32, device=dev) if want_grad else None
    ppos = torch.empty((n_t, H), dtype=torch.float32, device=dev) if want_grad else None
    nnz = csr.col.numel()
    algo = nnz * (4 * d + 4 * H + 4) + (n_t + 1) * 4 + n_t * (4 * width + 12 * H) + (n_t * (4 * d + 4 * H) if want_grad else 0) \
        + (n_t * 4 * d if agg is not None else 0)
    with on_device(dev), _timed("gat_fwd", dev, algo):
        check(_lib.load().allset_gat_fwd(1, nnz, ptr(_gat_order(csr, n_t)), ptr(csr.rowptr), ptr(csr.col), ptr(al), ptr(ar), ptr(x),
                                         _ld(x), float(slope), ptr(bias), RELU_ACTS[act], float(p), int(seed), ptr(seed_base),
                                         1 if concat else 0, ptr(y), max(width, 1), ptr(agg), d, ptr(aggpos), d, ptr(ppos), ptr(m),
                                         ptr(l), n_t, n_s, H, C, stream_of(dev)), "allset_gat_fwd")
    return y, agg, aggpos, ppos, m, l


def gat_bwd_stats(g: Tensor, aggpos: Tensor, ppos: Tensor, m: Tensor, l: Tensor, slope: float, agg: Optional[Tensor] = None,
                  y: Optional[Tensor] = None, bias: Optional[Tensor] = None, p: float = 0.0) -> Tuple[Tensor, Tensor]:
    """``(stats [n_t, H, 2] = {m + log(l + 1e-16), <agg, g>}, gar [n_t, H])`` from the gradient ``g`` at ``agg``.  ``agg`` as saved by
    the head-mean forward, or None: rebuilt from the concat form's ``y``, ``bias`` and ``p`` wherever ``g != 0``."""
    dev = require_device(g, aggpos, ppos, m, l, agg, y, bias)
    _f32(g, "gat_bwd_stats")
    g = _rowmajor(g)
    n_t, d = g.shape
    H = m.shape[1]
    if agg is None and y is None:
        raise _lib.AllSetHipError("gat_bwd_stats: give agg, or the forward's y to rebuild it from")
    src = agg if agg is not None else y
    if tuple(src.shape) != (n_t, d) or tuple(aggpos.shape) != (n_t, d):
        raise _lib.AllSetHipError(f"gat_bwd_stats: g {tuple(g.shape)} against rows of shape {tuple(src.shape)} / {tuple(aggpos.shape)}")
    stats = torch.empty((n_t, H, 2), dtype=torch.float32, device=dev)
    gar = torch.empty((n_t, H), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("gat_bwd_stats", dev, 3 * n_t * d * 4 + n_t * H * 24):
        check(_lib.load().allset_gat_bwd_stats(ptr(y), _ld(y) if y is not None else d, ptr(bias), float(p), ptr(agg), d, ptr(aggpos), d,
                                               ptr(ppos), ptr(g), _ld(g), ptr(m), ptr(l), float(slope), ptr(stats), ptr(gar), n_t, H,
                                               d // H, stream_of(dev)), "allset_gat_bwd_stats")
    return stats, gar


def gat_bwd_src(csrT: CSR, x: Tensor, al: Tensor, ar: Tensor, g: Tensor, stats: Tensor, slope: float) -> Tuple[Tensor, Tensor]:
    """``(gx [n_s, H*C], gal [n_s, H])`` in one gather pass over ``csrT`` (rows = sources, cols = targets)."""
    dev = require_device(csrT.rowptr, x, al, ar, g, stats)
    x, g, al, ar = _rowmajor(x), _rowmajor(g), al.contiguous(), ar.contiguous()
    n_s, d = x.shape
    n_t, H = ar.shape
    if n_s > csrT.n_rows or csrT.n_cols > n_t or g.shape[0] != n_t or g.shape[1] != d:
        raise _lib.AllSetHipError(f"gat_bwd_src: CSR of {csrT.n_rows} x {csrT.n_cols} against {n_s} sources / g {tuple(g.shape)}")
    gx = torch.empty((n_s, d), dtype=torch.float32, device=dev)
    gal = torch.empty((n_s, H), dtype=torch.float32, device=dev)
    nnz = csrT.col.numel()
    with on_device(dev), _timed("gat_bwd_src", dev, nnz * (4 * d + 12 * H + 4) + (n_s + 1) * 4 + n_s * (8 * d + 8 * H)):
        check(_lib.load().allset_gat_bwd_src(1, nnz, ptr(_gat_order(csrT, n_s)), ptr(csrT.rowptr), ptr(csrT.col), ptr(al), ptr(ar),
                                             ptr(x), _ld(x), ptr(g), _ld(g), ptr(stats), float(slope), ptr(gx), d, ptr(gal), n_s, n_t,
                                             H, d // H, stream_of(dev)), "allset_gat_bwd_src")
    return gx, gal


# ---- hypergraph attention of HCHA's HypergraphConv(use_attention=True) (csrc/hattn.hip) --------------------------------------------
HATTN_MAX_HEADS, HATTN_MAX_WIDTH = 64, 512


def hattn_coef(csr_v: CSR, pos: Tensor, av: Tensor, ae: Tensor, slope: float, p: float = 0.0, seed: int = 0,
               seed_base: Optional[Tensor] = None):
    """The attention coefficients over ``csr_v`` (rows = vertices, cols = hyperedges): ``(a_v, a_e, m, l)`` with ``a`` =
    softmax over each vertex's incidences of ``leaky_relu(av[v] + ae[e])`` times the coefficient dropout's ``keep / (1 - p)`` (hash
    mask keyed by edge-list position * H + head), f32[nnz, H] in ``csr_v``'s order and in the hyperedge-major order (``pos``: int32
    position of each ``csr_v`` position in that CSR); ``m`` / ``l`` f32[n_v, H] the softmax statistics."""
    dev = require_device(csr_v.rowptr, pos, av, ae)
    _f32(av, "hattn_coef av")
    _f32(ae, "hattn_coef ae")
    av, ae = av.contiguous(), ae.contiguous()
    n_v, H = av.shape
    n_e = ae.shape[0]
    nnz = csr_v.col.numel()
    if ae.shape[1] != H or n_v > csr_v.n_rows or csr_v.n_cols > n_e or pos.numel() != nnz:
        raise _lib.AllSetHipError(f"hattn_coef: av {tuple(av.shape)} / ae {tuple(ae.shape)} against a CSR of {csr_v.n_rows} x {csr_v.n_cols}")
    a_v = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    a_e = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    m = torch.empty((n_v, H), dtype=torch.float32, device=dev)
    l = torch.empty((n_v, H), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("hattn_coef", dev, nnz * (8 + 12 * H) + (n_v + 1) * 4 + n_v * 12 * H):
        check(_lib.load().allset_hattn_coef(nnz, ptr(csr_v.rowptr), ptr(csr_v.col), ptr(csr_v.perm), ptr(pos), ptr(av), ptr(ae),
                                            float(slope), float(p), int(seed), ptr(seed_base), ptr(a_v), ptr(a_e), ptr(m), ptr(l), n_v,
                                            n_e, H, stream_of(dev)), "allset_hattn_coef")
    return a_v, a_e, m, l


def hattn_hop(csr: CSR, w: Tensor, x: Tensor, heads: int, n_t: int, r: Optional[Tensor] = None, s: Optional[Tensor] = None,
              concat: bool = True, bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0, seed: int = 0,
              seed_base: Optional[Tensor] = None) -> Tensor:
    """``agg[t, h] = s[t] * sum_{j in row t} w[j, h] * r[col_j] * x[col_j, h]`` over ``csr`` (``w`` f32[nnz, H] in its order), then
    ``drop_p(act(agg + bias))`` with the heads side by side (``concat``) or averaged.  fp32 only."""
    dev = require_device(csr.rowptr, w, x, r, s, bias)
    for t, what in ((x, "x"), (w, "w"), (r, "r"), (s, "s"), (bias, "bias")):
        if t is not None:
            _f32(t, f"hattn_hop {what}")
    x, w = _rowmajor(x), w.contiguous()
    r = r.contiguous() if r is not None else None
    s = s.contiguous() if s is not None else None
    bias = bias.contiguous() if bias is not None else None
    n_s, d = x.shape
    H = int(heads)
    if H < 1 or d % H != 0 or d == 0:
        raise _lib.AllSetHipError(f"hattn_hop: width {d} does not split into {H} heads")
    C = d // H
    nnz = csr.col.numel()
    width = d if concat else C
    if tuple(w.shape) != (nnz, H):
        raise _lib.AllSetHipError(f"hattn_hop: w {tuple(w.shape)} against ({nnz}, {H})")
    if bias is not None and bias.numel() != width:
        raise _lib.AllSetHipError(f"hattn_hop: bias has {bias.numel()} entries for width {width}")
    if (r is not None and r.numel() < n_s) or (s is not None and s.numel() < n_t):
        raise _lib.AllSetHipError("hattn_hop: r / s shorter than the rows they scale")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"hattn_hop: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    y = torch.empty((n_t, width), dtype=torch.float32, device=dev)
    algo = nnz * (4 * d + 4 * H + 4 + (4 if r is not None else 0)) + (n_t + 1) * 4 + n_t * 4 * width
    with on_device(dev), _timed("hattn_hop", dev, algo):
        check(_lib.load().allset_hattn_hop(nnz, ptr(_gat_order(csr, n_t)), ptr(csr.rowptr), ptr(csr.col), ptr(w), ptr(r), ptr(s), ptr(x),
                                           _ld(x), ptr(bias), HCONV_ACTS[act], float(p), int(seed), ptr(seed_base), 1 if concat else 0,
                                           ptr(y), max(width, 1), n_t, n_s, H, C, stream_of(dev)), "allset_hattn_hop")
    return y


def hattn_bwd_vertex(csr_v: CSR, pos: Tensor, a_v: Tensor, av: Tensor, ae: Tensor, m: Tensor, l: Tensor, slope: float, z: Tensor,
                     g: Tensor, y: Tensor, gy: Tensor, D: Tensor, B: Tensor):
    """``(gz [n_v, H*C], gav [n_v, H], ge_e [nnz, H])``: the V->E hop's transpose, the gradient at ``av`` and the per-incidence
    gradient at the pre-activation logit in hyperedge-major order, in one gather pass over ``csr_v`` (see csrc/hattn.hip)."""
    dev = require_device(csr_v.rowptr, pos, a_v, av, ae, m, l, z, g, y, gy, D, B)
    z, g, y, gy = _rowmajor(z), _rowmajor(g), _rowmajor(y), _rowmajor(gy)
    n_v, d = z.shape
    n_e = y.shape[0]
    H = av.shape[1]
    nnz = csr_v.col.numel()
    if tuple(g.shape) != (n_v, d) or y.shape[1] != d or tuple(gy.shape) != (n_e, d) or n_v > csr_v.n_rows or csr_v.n_cols > n_e \
            or tuple(a_v.shape) != (nnz, H) or D.numel() < n_v or B.numel() < n_e or d % H != 0:
        raise _lib.AllSetHipError(f"hattn_bwd_vertex: z {tuple(z.shape)} / g {tuple(g.shape)} / y {tuple(y.shape)} / gy {tuple(gy.shape)} "
                                  f"against a CSR of {csr_v.n_rows} x {csr_v.n_cols}")
    gz = torch.empty((n_v, d), dtype=torch.float32, device=dev)
    t = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    gav = torch.empty((n_v, H), dtype=torch.float32, device=dev)
    ge_e = torch.empty((nnz, H), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("hattn_bwd_vertex", dev, nnz * (8 * d + 12 * H + 16) + (n_v + 1) * 4 + n_v * (12 * d + 8 * H)):
        check(_lib.load().allset_hattn_bwd_vertex(nnz, ptr(csr_v.rowptr), ptr(csr_v.col), ptr(pos), ptr(a_v), ptr(av.contiguous()),
                                                  ptr(ae.contiguous()), ptr(m), ptr(l), float(slope), ptr(z), _ld(z), ptr(g), _ld(g),
                                                  ptr(y), _ld(y), ptr(gy), _ld(gy), ptr(D.contiguous()), ptr(B.contiguous()), ptr(gz), d,
                                                  ptr(t), ptr(gav), ptr(ge_e), n_v, n_e, H, d // H, stream_of(dev)),
              "allset_hattn_bwd_vertex")
    return gz, gav, ge_e


def hattn_bwd_edge(csr_e: CSR, ge_e: Tensor, n_e: int) -> Tensor:
    """``gae[e, h] = sum_{j in row e} ge_e[j, h]`` over the hyperedge-major CSR's own positions."""
    dev = require_device(csr_e.rowptr, ge_e)
    nnz, H = ge_e.shape
    gae = torch.empty((n_e, H), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("hattn_bwd_edge", dev, nnz * 4 * H + (n_e + 1) * 4 + n_e * 4 * H):
        check(_lib.load().allset_hattn_bwd_edge(nnz, ptr(csr_e.rowptr), ptr(ge_e), ptr(gae), n_e, H, stream_of(dev)),
              "allset_hattn_bwd_edge")
    return gae


# ---- UniGCNII: the E->V hop with GCNII's initial-residual step (csrc/unigcn.hip) ---------------------------------------------------
UNIGCN_MAX_WIDTH = 512


def unigcn_hop_supported(xe: Tensor, x0: Tensor) -> bool:
    """Is the fused launch built for these operands?  fp32, width a multiple of 4 up to 512, 16-byte aligned rows."""
    d = xe.shape[1]
    return (xe.dtype == x0.dtype == torch.float32 and 0 < d <= UNIGCN_MAX_WIDTH and d % 4 == 0
            and all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= d and t.data_ptr() % 16 == 0 for t in (xe, x0)))


def unigcn_hop_fwd(csr: CSR, xe: Tensor, x0: Tensor, n_t: int, degV: Optional[Tensor], alpha: float, use_norm: bool,
                   variant: Optional[int] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """``(xi, t)``: ``xi[v] = (1 - alpha) * t[v] * a[v] + alpha * x0[v]`` with ``a[v] = degV[v] * sum_{j in row v} xe[col_j]`` over
    ``csr`` (rows = vertices) and ``t[v] = 1 / ||a[v]||`` (0 for a zero row) when ``use_norm``, else ``t`` is None (= ones).  One launch;
    raises where the width is not built (see :func:`unigcn_hop_supported`)."""
    dev = require_device(csr.rowptr, xe, x0, degV)
    _f32(xe, "unigcn_hop_fwd")
    _f32(x0, "unigcn_hop_fwd x0")
    xe, x0 = _rowmajor(xe), _rowmajor(x0)
    n_s, d = xe.shape
    if x0.shape != (n_t, d):
        raise _lib.AllSetHipError(f"unigcn_hop_fwd: x0 is {tuple(x0.shape)}, expected {(n_t, d)}")
    if degV is not None:
        _f32(degV, "unigcn_hop_fwd degV")
        degV = degV.contiguous()
        if degV.numel() < n_t:
            raise _lib.AllSetHipError(f"unigcn_hop_fwd: degV has {degV.numel()} entries for {n_t} output rows")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"unigcn_hop_fwd: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    xi = torch.empty((n_t, d), dtype=torch.float32, device=dev)
    t = torch.empty(n_t, dtype=torch.float32, device=dev) if use_norm else None
    nnz = csr.col.numel()
    if variant is None:
        variant = csr.variant("segreduce", n_t) if d <= 256 else 1
    order = csr.row_order if (variant == 1 and csr.row_order is not None and csr.row_order.numel() == n_t) else None
    algo = nnz * (4 * d + 4) + (n_t + 1) * 4 + 2 * n_t * 4 * d + n_t * 4 * (1 + int(use_norm))
    with on_device(dev), _timed("unigcn_hop_fwd", dev, algo):
        check(_lib.load().allset_unigcn_hop_fwd(variant, nnz, ptr(order), ptr(csr.rowptr), ptr(csr.col), ptr(degV), ptr(xe), _ld(xe),
                                                ptr(x0), _ld(x0), float(alpha), int(bool(use_norm)), ptr(xi), max(d, 1), ptr(t), n_t,
                                                n_s, d, stream_of(dev)), "allset_unigcn_hop_fwd")
    return xi, t


# ---- UniGNN: the E->V hop with the row tail, UniGAT's V->E hop with the attention logit (csrc/unignn.hip) ------------------------------
UNIGNN_MAX_WIDTH = 512


def unignn_hop_supported(xe: Tensor, xs: Optional[Tensor] = None) -> bool:
    """Is the fused E->V launch built for these operands?  fp32, width a multiple of 4 up to 512, 16-byte aligned rows."""
    d = xe.shape[1]
    ts = (xe,) if xs is None else (xe, xs)
    return (all(t.dtype == torch.float32 for t in ts) and 0 < d <= UNIGNN_MAX_WIDTH and d % 4 == 0
            and all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.stride(0) >= d and t.data_ptr() % 16 == 0 for t in ts))


def unignn_hop_fwd(csr: CSR, xe: Tensor, n_t: int, s: Optional[Tensor] = None, xs: Optional[Tensor] = None, c=1.0,
                   use_norm: bool = False, act: Optional[str] = None, p: float = 0.0, seed: int = 0,
                   seed_base: Optional[Tensor] = None, variant: Optional[int] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """``(y, t)``: ``y[v] = drop_p(act(t[v] * a[v]))`` with ``a[v] = s[v] * sum_{j in row v} xe[col_j] + c * xs[v]`` over ``csr`` (rows =
    vertices) and ``t[v] = 1 / ||a[v]||`` (0 for a zero row) when ``use_norm``, else ``t`` is None (= ones).  ``c``: a float, or a device
    fp32 tensor of one element (read by the kernel).  One launch; raises where the width is not built (:func:`unignn_hop_supported`)."""
    c_dev = c if torch.is_tensor(c) else None
    dev = require_device(csr.rowptr, xe, xs, s, c_dev)
    _f32(xe, "unignn_hop_fwd")
    xe = _rowmajor(xe)
    n_s, d = xe.shape
    if xs is not None:
        _f32(xs, "unignn_hop_fwd xs")
        xs = _rowmajor(xs)
        if xs.shape != (n_t, d):
            raise _lib.AllSetHipError(f"unignn_hop_fwd: xs is {tuple(xs.shape)}, expected {(n_t, d)}")
    if s is not None:
        _f32(s, "unignn_hop_fwd s")
        s = s.contiguous()
        if s.numel() < n_t:
            raise _lib.AllSetHipError(f"unignn_hop_fwd: s has {s.numel()} entries for {n_t} output rows")
    if c_dev is not None:
        _f32(c_dev, "unignn_hop_fwd c")
        if c_dev.numel() != 1:
            raise _lib.AllSetHipError(f"unignn_hop_fwd: c has {c_dev.numel()} elements, expected one")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"unignn_hop_fwd: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    y = torch.empty((n_t, d), dtype=torch.float32, device=dev)
    t = torch.empty(n_t, dtype=torch.float32, device=dev) if use_norm else None
    nnz = csr.col.numel()
    if variant is None:
        variant = csr.variant("segreduce", n_t) if d <= 256 else 1
    order = csr.row_order if (variant == 1 and csr.row_order is not None and csr.row_order.numel() == n_t) else None
    algo = (nnz * (4 * d + 4) + (n_t + 1) * 4 + n_t * 4 * d * (1 + int(xs is not None))
            + n_t * 4 * (int(s is not None) + int(bool(use_norm))))
    with on_device(dev), _timed("unignn_hop_fwd", dev, algo):
        check(_lib.load().allset_unignn_hop_fwd(variant, nnz, ptr(order), ptr(csr.rowptr), ptr(csr.col), ptr(s), ptr(xe), _ld(xe),
                                                ptr(xs), _ld(xs) if xs is not None else 0, 0.0 if c_dev is not None else float(c),
                                                ptr(c_dev), int(bool(use_norm)), RELU_ACTS[act], float(p), int(seed),
                                                ptr(seed_base), ptr(y), max(d, 1), ptr(t), n_t, n_s, d, stream_of(dev)),
              "allset_unignn_hop_fwd")
    return y, t


def unignn_v2e_att_supported(x: Tensor, heads: int) -> bool:
    """Is the fused V->E launch built?  fp32, ``heads`` heads of C channels with C a multiple of 4, heads * C up to 512, 16-byte rows."""
    d = x.shape[1]
    return (x.dtype == torch.float32 and heads > 0 and 0 < d <= UNIGNN_MAX_WIDTH and d % heads == 0 and (d // heads) % 4 == 0
            and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.stride(0) >= d and x.data_ptr() % 16 == 0)


def unignn_v2e_att_fwd(csr: CSR, x: Tensor, n_t: int, s: Optional[Tensor], att: Tensor, heads: int,
                       variant: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """``(xe, ae)``: ``xe[e] = s[e] * sum_{j in row e} x[col_j]`` over ``csr`` (rows = hyperedges) and ``ae[e, h] = <xe[e, h, :], att[h, :]>``
    (``att`` f32 of ``heads * C`` elements).  One launch; raises where the shape is not built (:func:`unignn_v2e_att_supported`)."""
    dev = require_device(csr.rowptr, x, s, att)
    _f32(x, "unignn_v2e_att_fwd")
    _f32(att, "unignn_v2e_att_fwd att")
    x = _rowmajor(x)
    att = att.reshape(-1).contiguous()
    if att.data_ptr() % 16 != 0:                 # (a view at an odd offset: the kernel reads att 16 bytes per lane; d floats, copied)
        att = att.clone()
    n_s, d = x.shape
    H = int(heads)
    if H <= 0 or d % H != 0 or att.numel() != d:
        raise _lib.AllSetHipError(f"unignn_v2e_att_fwd: width {d} / att of {att.numel()} elements do not fit {H} heads")
    if s is not None:
        _f32(s, "unignn_v2e_att_fwd s")
        s = s.contiguous()
        if s.numel() < n_t:
            raise _lib.AllSetHipError(f"unignn_v2e_att_fwd: s has {s.numel()} entries for {n_t} output rows")
    if n_t > csr.n_rows or csr.n_cols > n_s:
        raise _lib.AllSetHipError(f"unignn_v2e_att_fwd: CSR of {csr.n_rows} x {csr.n_cols} against {n_t} outputs / {n_s} gathered rows")
    xe = torch.empty((n_t, d), dtype=torch.float32, device=dev)
    ae = torch.empty((n_t, H), dtype=torch.float32, device=dev)
    nnz = csr.col.numel()
    if variant is None:
        variant = csr.variant("segreduce", n_t) if d <= 256 else 1
    order = csr.row_order if (variant == 1 and csr.row_order is not None and csr.row_order.numel() == n_t) else None
    algo = nnz * (4 * d + 4) + (n_t + 1) * 4 + n_t * (4 * d + 4 * H + 4 * int(s is not None)) + 4 * d
    with on_device(dev), _timed("unignn_v2e_att_fwd", dev, algo):
        check(_lib.load().allset_unignn_v2e_att_fwd(variant, nnz, ptr(order), ptr(csr.rowptr), ptr(csr.col), ptr(s), ptr(x), _ld(x),
                                                    ptr(att), ptr(xe), max(d, 1), ptr(ae), n_t, n_s, H, d // H, stream_of(dev)),
              "allset_unignn_v2e_att_fwd")
    return xe, ae


# ---- HyperGCN: the on-device Laplacian approximation and its two-pass hop (csrc/hypergcn.hip) -----------------------------------------
HYPERGCN_MAX_WIDTH = 256             # 16-byte lanes: multiples of 4 up to here
HYPERGCN_MAX_SCALAR_WIDTH = 64       # one column per lane: any width up to here (the class counts of the last layer)


def _rows16(*ts: Tensor) -> bool:
    return all(t.stride(1) == 1 and t.stride(0) % 4 == 0 and t.data_ptr() % 16 == 0 for t in ts)


def hypergcn_hop_supported(x: Tensor) -> bool:
    """Are the two hop launches built for this operand?  fp32; width a multiple of 4 up to 256 with 16-byte aligned rows, or any
    width up to 64."""
    d = x.shape[1]
    if x.dtype != torch.float32 or d <= 0 or x.stride(1) != 1 or x.stride(0) < d:
        return False
    return (d % 4 == 0 and d <= HYPERGCN_MAX_WIDTH and _rows16(x)) or d <= HYPERGCN_MAX_SCALAR_WIDTH


def hypergcn_project(z: Tensor, rv: Tensor) -> Tensor:
    """``p[v] = z[v] . rv`` (f32[n]); rows with equal values give equal bits."""
    dev = require_device(z, rv)
    _f32(z, "hypergcn_project")
    _f32(rv, "hypergcn_project rv")
    z = _rowmajor(z)
    rv = rv.reshape(-1).contiguous()
    n, d = z.shape
    if rv.numel() != d:
        raise _lib.AllSetHipError(f"hypergcn_project: rv has {rv.numel()} entries for width {d}")
    p = torch.empty(n, dtype=torch.float32, device=dev)
    with on_device(dev), _timed("hypergcn_project", dev, n * d * 4 + d * 4 + n * 4):
        check(_lib.load().allset_hypergcn_project(ptr(z), _ld(z), ptr(rv), ptr(p), n, d, stream_of(dev)), "allset_hypergcn_project")
    return p


def hypergcn_select(csr_e: CSR, p: Tensor, mediators: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(S, I, w, size)`` per row of the hyperedge-major ``csr_e``: the members at the first arg-max / arg-min of ``p`` in edge-list
    order (ties by ``csr_e.perm``), the weight 1 / (2k - 3) (mediators) or 1 / k, and the size k."""
    dev = require_device(csr_e.rowptr, p)
    _f32(p, "hypergcn_select")
    p = p.contiguous()
    n_e, n_v, nnz = csr_e.n_rows, csr_e.n_cols, csr_e.col.numel()
    if p.numel() < n_v:
        raise _lib.AllSetHipError(f"hypergcn_select: p has {p.numel()} entries for {n_v} vertices")
    S = torch.empty(n_e, dtype=torch.int32, device=dev)
    I = torch.empty(n_e, dtype=torch.int32, device=dev)
    size = torch.empty(n_e, dtype=torch.int32, device=dev)
    w = torch.empty(n_e, dtype=torch.float32, device=dev)
    with on_device(dev), _timed("hypergcn_select", dev, nnz * 12 + n_e * 20):
        check(_lib.load().allset_hypergcn_select(ptr(csr_e.rowptr), ptr(csr_e.col), ptr(csr_e.perm), ptr(p), int(bool(mediators)),
                                                 ptr(S), ptr(I), ptr(w), ptr(size), n_e, n_v, nnz, stream_of(dev)),
              "allset_hypergcn_select")
    return S, I, w, size


def hypergcn_degree(csr_v: CSR, S: Tensor, I: Tensor, w: Tensor, size: Tensor, mediators: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """``(dinv, selfc, colx)`` over the vertex-major ``csr_v``: ``D^-1/2``, the self coefficient of the E->V pass and, per incidence
    of ``csr_v``, the row of the per-hyperedge buffer that pass gathers (-1: none)."""
    dev = require_device(csr_v.rowptr, S, I, w, size)
    n_v, n_e, nnz = csr_v.n_rows, csr_v.n_cols, csr_v.col.numel()
    for t, dt, what in ((S, torch.int32, "S"), (I, torch.int32, "I"), (size, torch.int32, "size"), (w, torch.float32, "w")):
        if t.dtype != dt or t.numel() < n_e or not t.is_contiguous():
            raise _lib.AllSetHipError(f"hypergcn_degree: {what} must be contiguous {dt} with at least {n_e} entries")
    dinv = torch.empty(n_v, dtype=torch.float32, device=dev)
    selfc = torch.empty(n_v, dtype=torch.float32, device=dev)
    colx = torch.empty(nnz, dtype=torch.int32, device=dev)
    with on_device(dev), _timed("hypergcn_degree", dev, nnz * 24 + n_v * 12):
        check(_lib.load().allset_hypergcn_degree(ptr(csr_v.rowptr), ptr(csr_v.col), ptr(S), ptr(I), ptr(w), ptr(size),
                                                 int(bool(mediators)), ptr(dinv), ptr(selfc), ptr(colx), n_v, n_e, nnz, stream_of(dev)),
              "allset_hypergcn_degree")
    return dinv, selfc, colx


def hypergcn_v2e(csr_e: CSR, S: Tensor, I: Tensor, w: Tensor, dinv: Tensor, x: Tensor, mediators: bool) -> Tensor:
    """The per-hyperedge rows of one hop: f32[2 n_e, d] (``P_e``, ``Q_e`` interleaved) with mediators, f32[n_e, d] without."""
    dev = require_device(csr_e.rowptr, S, I, w, dinv, x)
    _f32(x, "hypergcn_v2e")
    x = _rowmajor(x)
    n_v, d = x.shape
    n_e, nnz = csr_e.n_rows, csr_e.col.numel()
    if csr_e.n_cols > n_v or dinv.numel() < n_v or min(S.numel(), I.numel(), w.numel()) < n_e:
        raise _lib.AllSetHipError(f"hypergcn_v2e: {n_v} feature rows / {dinv.numel()} dinv entries against a CSR of {n_e} x {csr_e.n_cols}")
    pq = torch.empty(((2 if mediators else 1) * n_e, d), dtype=torch.float32, device=dev)
    order = csr_e.row_order if (csr_e.row_order is not None and csr_e.row_order.numel() == n_e) else None
    algo = (nnz * (4 * d + 8) + (n_e + 1) * 4 if mediators else 2 * n_e * (4 * d + 4)) + 12 * n_e + pq.numel() * 4
    with on_device(dev), _timed("hypergcn_v2e", dev, algo):
        check(_lib.load().allset_hypergcn_v2e(int(bool(mediators)), nnz, ptr(order), ptr(csr_e.rowptr), ptr(csr_e.col), ptr(S), ptr(I),
                                              ptr(w), ptr(dinv), ptr(x), _ld(x), ptr(pq), max(d, 1), n_e, n_v, d, stream_of(dev)),
              "allset_hypergcn_v2e")
    return pq


def hypergcn_e2v(csr_v: CSR, colx: Tensor, pq: Tensor, dinv: Tensor, selfc: Tensor, x: Tensor, bias: Optional[Tensor] = None,
                 act: Optional[str] = None, p: float = 0.0, seed: int = 0, seed_base: Optional[Tensor] = None,
                 variant: Optional[int] = None) -> Tensor:
    """``y[v] = drop_p(act(dinv[v] * (selfc[v] * dinv[v] * x[v] + sum_{j in row v, colx_j >= 0} pq[colx_j]) + bias))`` over the
    vertex-major ``csr_v`` with ``colx`` in place of its columns."""
    dev = require_device(csr_v.rowptr, colx, pq, dinv, selfc, x, bias)
    _f32(x, "hypergcn_e2v")
    _f32(pq, "hypergcn_e2v pq")
    x, pq = _rowmajor(x), _rowmajor(pq)
    n_v, d = x.shape
    nnz = csr_v.col.numel()
    if n_v != csr_v.n_rows or pq.shape[1] != d or colx.numel() != nnz or colx.dtype != torch.int32 or dinv.numel() < n_v \
            or selfc.numel() < n_v:
        raise _lib.AllSetHipError(f"hypergcn_e2v: x {tuple(x.shape)} / pq {tuple(pq.shape)} / colx {colx.numel()} do not fit a CSR of "
                                  f"{csr_v.n_rows} rows and {nnz} incidences")
    if bias is not None:
        _f32(bias, "hypergcn_e2v bias")
        bias = bias.contiguous()
        if bias.numel() != d:
            raise _lib.AllSetHipError(f"hypergcn_e2v: bias has {bias.numel()} entries for width {d}")
    y = torch.empty((n_v, d), dtype=torch.float32, device=dev)
    flat_ok = d % 4 == 0 and d <= HYPERGCN_MAX_WIDTH and _rows16(x, pq)
    if variant is None:
        variant = csr_v.variant("segreduce", n_v) if flat_ok else 1
    order = csr_v.row_order if (variant == 1 and csr_v.row_order is not None and csr_v.row_order.numel() == n_v) else None
    algo = nnz * (4 * d + 4) + (n_v + 1) * 4 + 8 * n_v + 2 * n_v * 4 * d
    with on_device(dev), _timed("hypergcn_e2v", dev, algo):
        check(_lib.load().allset_hypergcn_e2v(variant, nnz, ptr(order), ptr(csr_v.rowptr), ptr(colx), ptr(pq), _ld(pq), pq.shape[0],
                                              ptr(dinv), ptr(selfc), ptr(x), _ld(x), ptr(bias), RELU_ACTS[act], float(p), int(seed),
                                              ptr(seed_base), ptr(y), max(d, 1), n_v, d, stream_of(dev)), "allset_hypergcn_e2v")
    return y


# ---- HAN baseline: the DGL-style attention hop and the semantic attention (csrc/han.hip) ---------------------------------------------
HAN_SEM_HIDDEN, HAN_SEM_MAX_WIDTH, HAN_SEM_MAX_PATHS = 128, 128, 32


def _pitch(t: Tensor, what: str) -> int:
    """Row pitch of a 2-D view whose rows are contiguous (a column block of a wider row-major buffer is one)."""
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
        raise _lib.AllSetHipError(f"{what}: rows must be contiguous (got strides {tuple(t.stride())})")
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1], 1)


def han_hop_fwd(rowptr: Tensor, col: Tensor, x: Tensor, el: Tensor, er: Tensor, heads: int, slope: float, bias: Optional[Tensor],
                p_att: float, seed: int, seed_base: Optional[Tensor], y: Tensor, want_grad: bool):
    """One HAN attention hop over a target-major CSR of ``n_dst`` rows whose ``col`` indexes ``n_src`` source rows (a bipartite
    block: the targets are the first source nodes; the full graph is ``n_src == n_dst``): ``x`` [n_src, H*C], ``el`` [n_src, H],
    ``er`` [n_dst, H], into ``y`` (a [n_dst, H*C] view with contiguous rows, e.g. a column block of the stacked buffer).  Returns
    ``(outpos, ppos, lse)``; ``outpos`` / ``ppos`` only with ``want_grad``."""
    dev = require_device(rowptr, col, x, el, er, bias, y)
    for t, what in ((x, "x"), (el, "el"), (er, "er"), (bias, "bias"), (y, "y")):
        if t is not None:
            _f32(t, f"han_hop_fwd {what}")
    x, el, er = _rowmajor(x), el.contiguous(), er.contiguous()
    n_src, d = x.shape
    n_dst = rowptr.numel() - 1
    H = int(heads)
    if H < 1 or d % H != 0 or d == 0:
        raise _lib.AllSetHipError(f"han_hop_fwd: width {d} does not split into {H} heads")
    if n_dst < 0 or tuple(el.shape) != (n_src, H) or tuple(er.shape) != (n_dst, H) or tuple(y.shape) != (n_dst, d):
        raise _lib.AllSetHipError(f"han_hop_fwd: el {tuple(el.shape)} / er {tuple(er.shape)} / y {tuple(y.shape)} / rowptr "
                                  f"{rowptr.numel()} against {n_src} source rows of width {d}, {H} heads")
    if bias is not None and bias.numel() != d:
        raise _lib.AllSetHipError(f"han_hop_fwd: bias has {bias.numel()} entries for width {d}")
    bias = bias.contiguous() if bias is not None else None
    lse = torch.empty((n_dst, H), dtype=torch.float32, device=dev)
    outpos = torch.empty((n_dst, d), dtype=torch.float32, device=dev) if want_grad else None
    ppos = torch.empty((n_dst, H), dtype=torch.float32, device=dev) if want_grad else None
    nnz = col.numel()
    algo = nnz * (4 * d + 4 * H + 4) + (n_dst + 1) * 4 + n_dst * (4 * d + 12 * H) + (n_dst * (4 * d + 4 * H) if want_grad else 0)
    with on_device(dev), _timed("han_hop_fwd", dev, algo):
        check(_lib.load().allset_han_block_hop_fwd(nnz, ptr(rowptr), ptr(col), ptr(el), ptr(er), ptr(x), _ld(x), float(slope), ptr(bias),
                                                   float(p_att), int(seed), ptr(seed_base), ptr(y), _pitch(y, "han_hop_fwd y"),
                                                   ptr(outpos), d, ptr(ppos), ptr(lse), n_dst, n_src, H, d // H, stream_of(dev)),
              "allset_han_block_hop_fwd")
    return outpos, ppos, lse


def han_hop_bwd_stats(y: Tensor, bias: Optional[Tensor], gy: Tensor, outpos: Tensor, ppos: Tensor, lse: Tensor, slope: float):
    """``(g [n_dst, H*C] = gy * elu'(y), stats [n_dst, H, 2] = {lse, <out, g>}, ger [n_dst, H])`` over the target rows; ``y`` and
    ``gy`` may be column blocks."""
    dev = require_device(y, bias, gy, outpos, ppos, lse)
    for t in (y, gy, outpos, ppos, lse):
        _f32(t, "han_hop_bwd_stats")
    n, d = y.shape
    H = lse.shape[1]
    if tuple(gy.shape) != (n, d) or tuple(outpos.shape) != (n, d):
        raise _lib.AllSetHipError(f"han_hop_bwd_stats: gy {tuple(gy.shape)} / outpos {tuple(outpos.shape)} against y {tuple(y.shape)}")
    g = torch.empty((n, d), dtype=torch.float32, device=dev)
    stats = torch.empty((n, H, 2), dtype=torch.float32, device=dev)
    ger = torch.empty((n, H), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("han_hop_bwd_stats", dev, 5 * n * d * 4 + n * H * 16):
        check(_lib.load().allset_han_block_hop_bwd_stats(ptr(y), _pitch(y, "han_hop_bwd_stats y"), ptr(bias), ptr(gy),
                                                         _pitch(gy, "han_hop_bwd_stats gy"), ptr(outpos), d, ptr(ppos), ptr(lse),
                                                         float(slope), ptr(g), d, ptr(stats), ptr(ger), n, H, d // H, stream_of(dev)),
              "allset_han_block_hop_bwd_stats")
    return g, stats, ger


def han_hop_bwd_src(rowptrT: Tensor, colT: Tensor, slotT: Tensor, x: Tensor, el: Tensor, er: Tensor, g: Tensor, stats: Tensor,
                    slope: float, p_att: float, seed: int, seed_base: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """``(gx [n_src, H*C], gel [n_src, H])`` in one gather pass over the source-major CSR (``n_src`` rows; ``g`` / ``stats`` / ``er``
    have ``n_dst`` rows); ``slotT`` regenerates the forward's edge mask."""
    dev = require_device(rowptrT, colT, slotT, x, el, er, g, stats)
    for t in (x, el, er, g, stats):
        _f32(t, "han_hop_bwd_src")
    x, g, el, er, stats = _rowmajor(x), _rowmajor(g), el.contiguous(), er.contiguous(), stats.contiguous()
    n_src, d = x.shape
    n_dst, H = er.shape
    if (tuple(g.shape) != (n_dst, d) or rowptrT.numel() != n_src + 1 or slotT.numel() != colT.numel() or tuple(stats.shape) != (n_dst, H, 2)
            or tuple(el.shape) != (n_src, H)):
        raise _lib.AllSetHipError(f"han_hop_bwd_src: g {tuple(g.shape)} / rowptrT {rowptrT.numel()} / slotT {slotT.numel()} against "
                                  f"{n_src} source and {n_dst} target rows of width {d}, {colT.numel()} edges")
    gx = torch.empty((n_src, d), dtype=torch.float32, device=dev)
    gel = torch.empty((n_src, H), dtype=torch.float32, device=dev)
    nnz = colT.numel()
    with on_device(dev), _timed("han_hop_bwd_src", dev, nnz * (4 * d + 12 * H + 8) + (n_src + 1) * 4 + n_src * (8 * d + 8 * H)):
        check(_lib.load().allset_han_block_hop_bwd_src(nnz, ptr(rowptrT), ptr(colT), ptr(slotT), ptr(el), ptr(er), ptr(x), _ld(x), ptr(g),
                                                       _ld(g), ptr(stats), float(slope), float(p_att), int(seed), ptr(seed_base), ptr(gx),
                                                       d, ptr(gel), n_dst, n_src, H, d // H, stream_of(dev)),
              "allset_han_block_hop_bwd_src")
    return gx, gel


def _han_sem_blocks(N: int, M: int) -> int:
    nb = c_int64_t(0)
    check(_lib.load().allset_han_sem_blocks(N, M, byref(nb)), "allset_han_sem_blocks")
    return nb.value


def han_sem_fwd(z: Tensor, W1: Tensor, b1: Tensor, q: Tensor) -> Tuple[Tensor, Tensor]:
    """``(out [N, D], wbeta [2, M] = {w, beta})`` from ``z`` [N, M, D] (contiguous), ``W1`` [128, D], ``b1`` [128], ``q`` [128]."""
    dev = require_device(z, W1, b1, q)
    for t in (z, W1, b1, q):
        _f32(t, "han_sem_fwd")
    if z.dim() != 3 or not z.is_contiguous():
        raise _lib.AllSetHipError(f"han_sem_fwd: z must be a contiguous [N, M, D] tensor (got {tuple(z.shape)}, strides {tuple(z.stride())})")
    N, M, D = z.shape
    hidden = W1.shape[0]
    if tuple(W1.shape) != (hidden, D) or b1.numel() != hidden or q.numel() != hidden:
        raise _lib.AllSetHipError(f"han_sem_fwd: W1 {tuple(W1.shape)} / b1 {b1.numel()} / q {q.numel()} against width {D}")
    W1, b1, q = W1.contiguous(), b1.contiguous(), q.contiguous()
    part = torch.empty((_han_sem_blocks(N, M), M), dtype=torch.float32, device=dev)
    wbeta = torch.empty((2, M), dtype=torch.float32, device=dev)
    out = torch.empty((N, D), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("han_sem_fwd", dev, 2 * 4 * N * M * D + 4 * N * D):
        check(_lib.load().allset_han_sem_fwd(ptr(z), ptr(W1), ptr(b1), ptr(q), ptr(part), ptr(wbeta), ptr(out), N, M, D, hidden,
                                             stream_of(dev)), "allset_han_sem_fwd")
    return out, wbeta


def han_sem_bwd(z: Tensor, W1: Tensor, b1: Tensor, q: Tensor, wbeta: Tensor, gout: Tensor):
    """``(gz [N, M, D], gW1 [128, D], gb1 [128], gq [128])``; the hidden is recomputed, parameter gradients by block reduction."""
    dev = require_device(z, W1, b1, q, wbeta, gout)
    for t in (z, W1, b1, q, wbeta, gout):
        _f32(t, "han_sem_bwd")
    N, M, D = z.shape
    hidden = W1.shape[0]
    if tuple(gout.shape) != (N, D) or tuple(wbeta.shape) != (2, M) or not wbeta.is_contiguous() or not z.is_contiguous():
        raise _lib.AllSetHipError(f"han_sem_bwd: gout {tuple(gout.shape)} / wbeta {tuple(wbeta.shape)} against z {tuple(z.shape)}")
    W1, b1, q, gout = W1.contiguous(), b1.contiguous(), q.contiguous(), gout.contiguous()
    nb = _han_sem_blocks(N, M)
    P = hidden * D + 2 * hidden
    part = torch.empty((nb, M), dtype=torch.float32, device=dev)
    gsm = torch.empty((M,), dtype=torch.float32, device=dev)
    gz = torch.empty((N, M, D), dtype=torch.float32, device=dev)
    ppart = torch.empty((nb, P), dtype=torch.float32, device=dev)
    gparams = torch.empty((P,), dtype=torch.float32, device=dev)
    with on_device(dev), _timed("han_sem_bwd", dev, 3 * 4 * N * M * D + 2 * 4 * N * D + nb * P * 4):
        check(_lib.load().allset_han_sem_bwd(ptr(z), ptr(W1), ptr(b1), ptr(q), ptr(wbeta), ptr(gout), ptr(part), ptr(gsm), ptr(gz),
                                             ptr(ppart), ptr(gparams), N, M, D, hidden, stream_of(dev)), "allset_han_sem_bwd")
    return gz, gparams[:hidden * D].view(hidden, D), gparams[hidden * D:hidden * D + hidden], gparams[hidden * D + hidden:]


# ---- mini-batch HAN: the metapath random walk, the block construction and the bipartite hop (csrc/han_sample.hip) ----------------------
HAN_MAX_WALKS = 64
HAN_MAX_HOPS = 8


def _i32(t: Tensor, what: str) -> Tensor:
    if t.dtype != torch.int32:
        raise _lib.AllSetHipError(f"{what}: int32 required (got {t.dtype})")
    return t.contiguous()


def _han_counter(who: str, counter, counter_add: int):
    """``(device tensor or None, 64-bit value)`` of a walk's step counter: an int travels by value (``counter_add`` added here); a
    1-element uint64 / int64 DEVICE tensor is read by the kernel, which adds ``counter_add`` (64-bit wrap either way)."""
    add = int(counter_add) & 0xFFFFFFFFFFFFFFFF
    if not torch.is_tensor(counter):
        return None, (int(counter) + add) & 0xFFFFFFFFFFFFFFFF
    if counter.dtype not in (torch.uint64, torch.int64) or counter.numel() != 1:
        raise _lib.AllSetHipError(f"{who}: a counter tensor is ONE uint64 / int64 element (got {counter.dtype}, {counter.numel()} "
                                  "elements)")
    if not counter.is_cuda:
        raise _lib.AllSetHipError(f"{who}: a counter tensor must live on the device (got a CPU tensor); pass an int for a host counter")
    return counter, add


def han_walk(metapath: int, csr_a: CSR, csr_b: CSR, id_base: int, seeds: Tensor, k: int, seed: int, counter, counter_add: int = 0) -> Tensor:
    """``k`` two-hop walks per seed over CSR ``csr_a`` then ``csr_b`` (the binarised incidence in the metapath's orientation):
    endpoints int32[B, k] in global ids, -1 where the walk terminates.  ``seeds`` int32[B] global ids.  ``counter``: an int, or a
    1-element uint64 / int64 device tensor the kernel reads (the effective counter is ``counter + counter_add`` mod 2^64; equal
    effective counters give bit-identical walks)."""
    ctensor, cval = _han_counter("han_walk", counter, counter_add)
    dev = require_device(csr_a.rowptr, csr_a.col, csr_b.rowptr, csr_b.col, seeds, ctensor)
    seeds = _i32(seeds, "han_walk seeds")
    B, k = seeds.numel(), int(k)
    if csr_a.n_cols != csr_b.n_rows or csr_b.n_cols != csr_a.n_rows:
        raise _lib.AllSetHipError(f"han_walk: CSR A {csr_a.n_rows} x {csr_a.n_cols} and CSR B {csr_b.n_rows} x {csr_b.n_cols} are not "
                                  "the two orientations of one incidence")
    out = torch.empty((B, max(k, 0)), dtype=torch.int32, device=dev)
    if ctensor is not None:
        with on_device(dev), _timed("han_walk", dev, B * max(k, 0) * 20 + B * 4):
            check(_lib.load().allset_han_walk_dc(int(metapath), ptr(csr_a.rowptr), ptr(csr_a.col), ptr(csr_b.rowptr), ptr(csr_b.col),
                                                 csr_a.n_rows, csr_b.n_rows, int(id_base), ptr(seeds), B, k,
                                                 int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(ctensor), cval, ptr(out), stream_of(dev)),
                  "allset_han_walk_dc")
        return out
    counter = cval
    with on_device(dev), _timed("han_walk", dev, B * max(k, 0) * 20 + B * 4):
        check(_lib.load().allset_han_walk(int(metapath), ptr(csr_a.rowptr), ptr(csr_a.col), ptr(csr_b.rowptr), ptr(csr_b.col),
                                          csr_a.n_rows, csr_b.n_rows, int(id_base), ptr(seeds), B, k,
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF, ptr(out), stream_of(dev)),
              "allset_han_walk")
    return out


def han_walk_typed(metapath_index: int, csrs: Sequence[CSR], seeds: Tensor, k: int, seed: int, counter, counter_add: int = 0) -> Tensor:
    """``k`` walks per seed along the chain ``csrs`` of relation CSRs (rows = source ids, as ``HeteroGraph.csr`` builds them;
    duplicate edges kept): endpoints int32[B, k] in the ids of the last relation's destination type, -1 where the walk terminates.
    ``seeds`` int32[B] ids of the first relation's source type.  For two hops, bit-identical to :func:`han_walk` with ``id_base`` 0.
    ``counter`` / ``counter_add`` as there."""
    ctensor, cval = _han_counter("han_walk_typed", counter, counter_add)
    csrs = list(csrs)
    L = len(csrs)
    if not 1 <= L <= HAN_MAX_HOPS:
        raise _lib.AllSetHipError(f"han_walk_typed: a metapath of {L} hops; the walk kernel is built for 1 to HAN_MAX_HOPS = "
                                  f"{HAN_MAX_HOPS}")
    dev = require_device(*[t for c in csrs for t in (c.rowptr, c.col)], seeds, ctensor)
    seeds = _i32(seeds, "han_walk_typed seeds")
    for i, c in enumerate(csrs):
        _i32(c.rowptr, f"han_walk_typed rowptr of hop {i}"), _i32(c.col, f"han_walk_typed col of hop {i}")
        if not (c.rowptr.is_contiguous() and c.col.is_contiguous()) or c.rowptr.numel() != c.n_rows + 1:
            raise _lib.AllSetHipError(f"han_walk_typed: hop {i}: rowptr of {c.rowptr.numel()} entries for {c.n_rows} rows, or a "
                                      "non-contiguous CSR")
        if i + 1 < L and c.n_cols != csrs[i + 1].n_rows:
            raise _lib.AllSetHipError(f"han_walk_typed: hop {i} leads to {c.n_cols} nodes but hop {i + 1} starts from "
                                      f"{csrs[i + 1].n_rows}: the chain's relations do not meet")
    B, k = seeds.numel(), int(k)
    out = torch.empty((B, max(k, 0)), dtype=torch.int32, device=dev)
    rowptrs = (c_void_p * L)(*[ptr(c.rowptr) for c in csrs])
    cols = (c_void_p * L)(*[ptr(c.col) if c.col.numel() else None for c in csrs])
    n_rows = (c_int64_t * L)(*[c.n_rows for c in csrs])
    # per walk and hop two row pointers and one column, then the endpoint
    if ctensor is not None:
        with on_device(dev), _timed("han_walk_typed", dev, B * max(k, 0) * (12 * L + 4) + B * 4):
            check(_lib.load().allset_han_walk_typed_dc(int(metapath_index), L, rowptrs, cols, n_rows, ptr(seeds), B, k,
                                                       int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(ctensor), cval, ptr(out), stream_of(dev)),
                  "allset_han_walk_typed_dc")
        return out
    counter = cval
    with on_device(dev), _timed("han_walk_typed", dev, B * max(k, 0) * (12 * L + 4) + B * 4):
        check(_lib.load().allset_han_walk_typed(int(metapath_index), L, rowptrs, cols, n_rows, ptr(seeds), B, k,
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(counter) & 0xFFFFFFFFFFFFFFFF, ptr(out),
                                                stream_of(dev)), "allset_han_walk_typed")
    return out


def han_block_rows(endpoints: Tensor, seeds: Tensor, seeds_sorted: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """``(rows, extra, counts)``: per seed the distinct endpoints ascending, then the self-loop, then -1 (int32[B, k + 1]); the same
    with seed-set members and padding as INT32_MAX; the row lengths."""
    dev = require_device(endpoints, seeds, seeds_sorted)
    endpoints, seeds, seeds_sorted = _i32(endpoints, "han_block_rows"), _i32(seeds, "han_block_rows"), _i32(seeds_sorted, "han_block_rows")
    if endpoints.dim() != 2 or endpoints.shape[0] != seeds.numel() or seeds_sorted.numel() != seeds.numel():
        raise _lib.AllSetHipError(f"han_block_rows: endpoints {tuple(endpoints.shape)} against {seeds.numel()} seeds")
    B, k = endpoints.shape
    rows = torch.empty((B, k + 1), dtype=torch.int32, device=dev)
    extra = torch.empty((B, k + 1), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    with on_device(dev), _timed("han_block_rows", dev, B * (k + 2 * (k + 1) + 2) * 4):
        check(_lib.load().allset_han_block_rows(ptr(endpoints), ptr(seeds), ptr(seeds_sorted), B, k, ptr(rows), ptr(extra), ptr(counts),
                                                stream_of(dev)), "allset_han_block_rows")
    return rows, extra, counts


def han_block_compact(rows: Tensor, counts: Tensor, rowptr: Tensor, seeds_sorted: Tensor, seed_perm: Tensor, uniq: Tensor, n_extra: int,
                      nnz: int) -> Tuple[Tensor, Tensor]:
    """``(col, dst)`` int32[nnz]: the target-major CSR's block-local source ids and the target of every slot."""
    dev = require_device(rows, counts, rowptr, seeds_sorted, seed_perm, uniq)
    for t in (rows, counts, rowptr, seeds_sorted, seed_perm, uniq):
        _i32(t, "han_block_compact")
    B, k = rows.shape[0], rows.shape[1] - 1
    if (not rows.is_contiguous() or counts.numel() != B or rowptr.numel() != B + 1 or seeds_sorted.numel() != B or seed_perm.numel() != B
            or uniq.numel() < n_extra):
        raise _lib.AllSetHipError(f"han_block_compact: rows {tuple(rows.shape)} / counts {counts.numel()} / rowptr {rowptr.numel()} / "
                                  f"uniq {uniq.numel()} for {n_extra} non-seed nodes")
    col = torch.empty((nnz,), dtype=torch.int32, device=dev)
    dst = torch.empty((nnz,), dtype=torch.int32, device=dev)
    with on_device(dev), _timed("han_block_compact", dev, B * (k + 1) * 4 + nnz * 8):
        check(_lib.load().allset_han_block_compact(ptr(rows), ptr(counts.contiguous()), ptr(rowptr.contiguous()), ptr(seeds_sorted.contiguous()),
                                                   ptr(seed_perm.contiguous()), ptr(uniq.contiguous()), int(n_extra), B, k, int(nnz), ptr(col),
                                                   ptr(dst), stream_of(dev)), "allset_han_block_compact")
    return col, dst


_HAN_FIXED_MAX_SLAB: Optional[int] = None


def han_fixed_max_slab() -> int:
    """The largest slab ``B * (k + 1)`` the fixed-capacity block kernels are built for."""
    global _HAN_FIXED_MAX_SLAB
    if _HAN_FIXED_MAX_SLAB is None:
        n = c_int64_t(0)
        check(_lib.load().allset_han_block_fixed_max_slab(byref(n)), "allset_han_block_fixed_max_slab")
        _HAN_FIXED_MAX_SLAB = n.value
    return _HAN_FIXED_MAX_SLAB


def han_fixed_check(B: int, k: int) -> int:
    """The capacity ``B * (k + 1)`` of a fixed block; refuses (host only) an empty batch, ``k`` outside the walk's and a slab beyond
    :func:`han_fixed_max_slab`."""
    B, k = int(B), int(k)
    if B < 1:
        raise _lib.AllSetHipError("a fixed-capacity block needs at least one seed (B == 0)")
    if not 1 <= k <= HAN_MAX_WALKS:
        raise _lib.AllSetHipError(f"a fixed-capacity block: k = {k} walks per seed outside [1, {HAN_MAX_WALKS}]")
    cap, limit = B * (k + 1), han_fixed_max_slab()
    if cap > limit:
        raise _lib.AllSetHipError(f"a fixed-capacity block of B * (k + 1) = {B} * {k + 1} = {cap} slots exceeds the built maximum "
                                  f"({limit}): not built")
    return cap


def han_block_relabel(counts: Tensor, extra_sorted: Tensor, seeds_sorted: Tensor, k: int, status: Optional[Tensor] = None
                      ) -> Tuple[Tensor, Tensor, Tensor]:
    """``(rowptr int32[B + 1], uniq int32[cap], sizes int32[2] = {nnz, n_extra})`` from the row lengths and the SORTED extra slab
    (``cap = B * (k + 1)`` entries), one launch; ``status`` (int32[1]) is set to 1 when ``seeds_sorted`` holds a duplicate."""
    dev = require_device(counts, extra_sorted, seeds_sorted, status)
    for t in (counts, extra_sorted, seeds_sorted) + ((status,) if status is not None else ()):
        _i32(t, "han_block_relabel")
    B = counts.numel()
    cap = han_fixed_check(B, k)
    if extra_sorted.numel() != cap or seeds_sorted.numel() != B or (status is not None and status.numel() != 1) or not (
            counts.is_contiguous() and extra_sorted.is_contiguous() and seeds_sorted.is_contiguous()):
        raise _lib.AllSetHipError(f"han_block_relabel: extra slab of {extra_sorted.numel()} / {seeds_sorted.numel()} sorted seeds for "
                                  f"B = {B}, k = {k}, or a non-contiguous tensor")
    rowptr = torch.empty((B + 1,), dtype=torch.int32, device=dev)
    uniq = torch.empty((cap,), dtype=torch.int32, device=dev)
    sizes = torch.empty((2,), dtype=torch.int32, device=dev)
    with on_device(dev), _timed("han_block_relabel", dev, (2 * B + 2 * cap) * 4):
        check(_lib.load().allset_han_block_relabel(ptr(counts), ptr(extra_sorted), ptr(seeds_sorted), B, int(k), ptr(rowptr), ptr(uniq),
                                                   ptr(sizes), ptr(status), stream_of(dev)), "allset_han_block_relabel")
    return rowptr, uniq, sizes


def han_block_compact_fixed(rows: Tensor, counts: Tensor, rowptr: Tensor, seeds: Tensor, seeds_sorted: Tensor, seed_order: Tensor,
                            uniq: Tensor, sizes: Tensor) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """``(col, dst, key int32[cap], src_ids int64[cap])``: :func:`han_block_compact` with the sizes on the device and every slot
    written (padding: ``col = dst = 0``, ``key = cap``; ``src_ids``: the seeds, the distinct other nodes, then the first seed)."""
    dev = require_device(rows, counts, rowptr, seeds, seeds_sorted, seed_order, uniq, sizes)
    for t in (rows, counts, rowptr, seeds, seeds_sorted, uniq, sizes):
        _i32(t, "han_block_compact_fixed")
    if rows.dim() != 2 or seed_order.dtype != torch.int64:
        raise _lib.AllSetHipError(f"han_block_compact_fixed: rows {tuple(rows.shape)}, seed_order {seed_order.dtype} (int64: the sort's "
                                  "permutation)")
    B, k = rows.shape[0], rows.shape[1] - 1
    cap = han_fixed_check(B, k)
    ts = (rows, counts, rowptr, seeds, seeds_sorted, seed_order, uniq, sizes)
    if ([t.numel() for t in ts] != [cap, B, B + 1, B, B, B, cap, 2]) or not all(t.is_contiguous() for t in ts):
        raise _lib.AllSetHipError(f"han_block_compact_fixed: sizes {[t.numel() for t in ts]} for B = {B}, k = {k}, or a non-contiguous "
                                  "tensor")
    col = torch.empty((cap,), dtype=torch.int32, device=dev)
    dst = torch.empty((cap,), dtype=torch.int32, device=dev)
    key = torch.empty((cap,), dtype=torch.int32, device=dev)
    src_ids = torch.empty((cap,), dtype=torch.int64, device=dev)
    with on_device(dev), _timed("han_block_compact_fixed", dev, cap * 28):
        check(_lib.load().allset_han_block_compact_fixed(ptr(rows), ptr(counts), ptr(rowptr), ptr(seeds), ptr(seeds_sorted),
                                                         ptr(seed_order), ptr(uniq), ptr(sizes), B, k, ptr(col), ptr(dst), ptr(key),
                                                         ptr(src_ids), stream_of(dev)), "allset_han_block_compact_fixed")
    return col, dst, key, src_ids


def han_block_transpose(keys_sorted: Tensor, perm: Tensor, dst: Tensor, B: int, k: int) -> Tuple[Tensor, Tensor, Tensor]:
    """``(rowptrT int32[cap + 1], colT, slotT int32[cap])`` of the source-major CSR from the stably sorted keys of
    :func:`han_block_compact_fixed` and the sort's permutation (int64), one launch."""
    dev = require_device(keys_sorted, perm, dst)
    _i32(keys_sorted, "han_block_transpose"), _i32(dst, "han_block_transpose")
    cap = han_fixed_check(B, k)
    if perm.dtype != torch.int64 or [keys_sorted.numel(), perm.numel(), dst.numel()] != [cap] * 3 or not (
            keys_sorted.is_contiguous() and perm.is_contiguous() and dst.is_contiguous()):
        raise _lib.AllSetHipError(f"han_block_transpose: keys {keys_sorted.numel()} / perm {perm.numel()} ({perm.dtype}) / dst "
                                  f"{dst.numel()} for a capacity of {cap}, or a non-contiguous tensor")
    rowptrT = torch.empty((cap + 1,), dtype=torch.int32, device=dev)
    colT = torch.empty((cap,), dtype=torch.int32, device=dev)
    slotT = torch.empty((cap,), dtype=torch.int32, device=dev)
    with on_device(dev), _timed("han_block_transpose", dev, cap * 28):
        check(_lib.load().allset_han_block_transpose(ptr(keys_sorted), ptr(perm), ptr(dst), int(B), int(k), ptr(rowptrT), ptr(colT),
                                                     ptr(slotT), stream_of(dev)), "allset_han_block_transpose")
    return rowptrT, colT, slotT
