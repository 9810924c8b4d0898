"""Differentiable aggregation operators backed by the HIP kernels (``torch.autograd.Function``
wrappers over ``ops.py``).  These two functions are the whole "propagate" step of the reference:

* ``deepsets_aggregate``  == ``HalfNLHconv.propagate`` -> ``message`` -> ``aggregate``  (layers.py:633-656)
* ``pma_aggregate``       == ``PMA.propagate`` -> ``message`` -> ``aggregate``           (layers.py:145,168-194)

Backward passes are kernels too (same segreduce kernel on the transposed CSR; one-gather-pass PMA
backward) -- no autograd graph over per-incidence temporaries exists.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib, _memo, ops
from .dense import PackedRows
from ._lib import MAX, MEAN, MIN, REDUCE_CODES, SUM
from .incidence import Incidence, LeaveOneOutIncidence

Tensor = torch.Tensor


def _variant(csr, kind: str, n_rows: int, x: Tensor, heads: int = 1) -> int:
    """Short-row kernel (2) only where it is built: 16-byte packets covering the whole row in one chunk."""
    es = x.element_size()
    wide = 16 // es
    d = x.shape[1]
    ok = (d % wide == 0 and d <= 64 * wide and x.stride(0) % wide == 0 and x.data_ptr() % 16 == 0
          and (d // max(heads, 1)) % wide == 0)
    if not ok:
        return 1
    if d * es <= 128 and csr.max_deg <= 512:
        # rows of at most one cache line (the column-sharded layer, dist.py): a wavefront per row leaves most lanes
        # idle; the short-row kernel packs 64 / (d / wide) rows into each (profiles/r01_colshard_kernels.txt)
        return 2
    return csr.variant(kind, n_rows)


def _sizes(csr, x: Tensor, heads: int = 1):
    """``CSR.sizes`` (long-row list + compacted short rows, ops.SizeSplit) where it pays and the short-row kernel exists: rows of
    at most one cache line.  ``ALLSET_SIZE_SPLIT=0`` turns it off."""
    import os
    if getattr(csr, "sizes", None) is None or os.environ.get("ALLSET_SIZE_SPLIT", "1") == "0":
        return None
    es = x.element_size()
    wide = 16 // es
    d = x.shape[1]
    ok = (d % wide == 0 and d * es <= 128 and x.stride(0) % wide == 0 and x.data_ptr() % 16 == 0 and (d // max(heads, 1)) % wide == 0)
    return csr.sizes if ok else None


def _split(csr, x: Tensor, heads: int = 1) -> int:
    """``CSR.short_tail`` if the short-row kernel exists for this feature layout, else -1 (single launch)."""
    if csr.short_tail <= 0:
        return -1
    es = x.element_size()
    wide = 16 // es
    d = x.shape[1]
    ok = (d % wide == 0 and d <= 64 * wide and x.stride(0) % wide == 0 and x.data_ptr() % 16 == 0
          and (d // max(heads, 1)) % wide == 0)
    return csr.short_tail if ok else -1


def _check_rows(x: Tensor, inc: Incidence) -> None:
    """The gathered matrix must cover every source id (PyG's index_select would raise otherwise) and
    may not have more rows than the transposed CSR (its backward produces one row per CSR row)."""
    if not (inc.src_extent <= x.shape[0] <= inc.n_src):
        raise ValueError(f"source matrix has {x.shape[0]} rows; incidence needs between {inc.src_extent} "
                         f"and {inc.n_src}")


class _RouteWeights(torch.autograd.Function):
    """``w[perm]`` for a PERMUTATION ``perm`` (edge-list order -> CSR order of a trainable per-incidence weight, LearnMask):
    the backward of a permutation is the gather by its inverse -- torch's advanced-indexing backward is a sort-based
    ``index_put`` (several radix-sort passes over nnz keys per call, ~1 ms at nnz = 16M)."""

    @staticmethod
    def forward(ctx, w, perm, inv_perm):
        ctx.save_for_backward(inv_perm)
        return w.index_select(0, perm)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (inv_perm,) = ctx.saved_tensors
        return g.index_select(0, inv_perm), None, None


def _routed(norm: Tensor, inc: Incidence, dst: bool) -> Tensor:
    """``norm`` (edge-list order, requires grad) in the order of ``inc.by_dst`` / ``inc.by_src``.

    A NON-LEAF norm (SetGNN's ``Importance * norm``, a fresh tensor per forward) keeps the routed copy on itself (``_memo``) per
    (CSR object, grad mode): the V->E and E->V convs of a layer share one routing and autograd sums their gradients; the
    cache dies with that forward's tensor.  A LEAF (an ``nn.Parameter`` handed straight to ``deepsets_aggregate``) is never
    cached: it outlives the forward, the optimizer updates it in place, a hit would replay the first call's values and graph
    (and keep it alive through AccumulateGrad -> tensor -> cache).  Routing is one gather, 0.2 ms at nnz = 16M."""
    csr = inc.by_dst if dst else inc.by_src
    perm, inv = (inc.perm_dst_long(), inc.inv_perm_dst()) if dst else (inc.perm_src_long(), inc.inv_perm_src())
    if norm.grad_fn is None:
        return _RouteWeights.apply(norm.reshape(-1).to(torch.float32), perm, inv)
    return _memo.get(norm, "routed", (id(csr), torch.is_grad_enabled()), lambda: _RouteWeights.apply(norm.reshape(-1).to(torch.float32), perm, inv))


_PACKED_GATHER = True


def set_packed_gather(on: bool) -> None:
    """Module switch (default on; A/B runs and tests): whether a forward aggregation whose caller hints at a mostly-zero table
    (``deepsets_aggregate(..., packed_rows=True)``) gathers packed nonzero rows.  The results are bitwise the
    same either way."""
    global _PACKED_GATHER
    _PACKED_GATHER = bool(on)


def packed_gather() -> bool:
    return _PACKED_GATHER


# Per direction of a layer, as tools/cell_gather_bench.py decided it: the cell gather passed the kill criterion
# over the E->V CSR and missed it over the V->E one (the mask gather's own repeats scatter too much there), so V->E keeps the mask rows.
# ``None``: an aggregation whose caller named no direction (a bare ``HalfNLHconv``, ``deepsets_aggregate``).
_PACKED_FORMAT = {"v2e": "mask", "e2v": "cells", None: "cells"}
_PACKED_DIRECTION = None


def set_packed_format(fmt: str, direction: Optional[str] = None) -> None:
    """Module switch beside :func:`set_packed_gather`: which packed rows a forward aggregation gathers --
    ``"cells"`` (every occupied element with its column beside it, expanded per occupied element) or ``"mask"`` (occupancy mask +
    values, expanded per column).  ``direction``: ``"v2e"`` / ``"e2v"`` sets it for that half of a layer (:func:`packed_direction`),
    ``None`` for every aggregation.  Every fall-back condition is the same for both formats, and so are the results, bit for bit."""
    ops.packed_format_entry(fmt, "set_packed_format")
    if direction not in (None, "v2e", "e2v"):
        raise ValueError(f"set_packed_format: direction must be None, 'v2e' or 'e2v', got {direction!r}")
    for key in ((direction,) if direction is not None else tuple(_PACKED_FORMAT)):
        _PACKED_FORMAT[key] = fmt


def packed_format(direction: Optional[str] = None) -> str:
    """The format of ``direction``, or of the direction the caller is in (:func:`packed_direction`)."""
    return _PACKED_FORMAT[direction if direction is not None else _PACKED_DIRECTION]


class packed_direction:
    """``with packed_direction("v2e"):`` -- the aggregations inside belong to that half of a V->E->V layer and gather the packed
    format chosen for it.  Host-side state only: nothing here touches the device, the step still captures."""

    def __init__(self, direction: str):
        if direction not in ("v2e", "e2v"):
            raise ValueError(f"packed_direction: 'v2e' or 'e2v', got {direction!r}")
        self.direction = direction

    def __enter__(self):
        global _PACKED_DIRECTION
        self.was, _PACKED_DIRECTION = _PACKED_DIRECTION, self.direction

    def __exit__(self, *exc):
        global _PACKED_DIRECTION
        _PACKED_DIRECTION = self.was


_PACKED_EPILOGUE = "auto"
# "auto": the fused Linear writes the packed rows itself from this many rows upward.  Below a few thousand rows both forms are bound
# by their launches (DESIGN.md section 4.5 has the measured crossover); tests/test_gpu_packed_gather.py pins pack_rows at 500 rows.
PACKED_EPILOGUE_MIN_ROWS = 16384


def set_packed_epilogue(mode: str) -> None:
    """Module switch beside :func:`set_packed_gather` (which still turns everything off): whether the last ``f_enc`` Linear in front
    of a packed gather writes the packed rows from its own epilogue (``dense.fused_norm_linear_packed``) instead of a dense table
    that ``ops.pack_rows`` then packs.  ``"auto"`` (default): from ``PACKED_EPILOGUE_MIN_ROWS`` rows upward; ``"on"``: at any size
    (tests); ``"off"``: never.  The results are bitwise the same either way."""
    global _PACKED_EPILOGUE
    if mode not in ("auto", "on", "off"):
        raise ValueError(f"set_packed_epilogue: mode must be 'auto', 'on' or 'off', got {mode!r}")
    _PACKED_EPILOGUE = mode


def packed_epilogue() -> str:
    return _PACKED_EPILOGUE


class _RowsToCome:
    """What ``_takes_packed`` reads of a table that does not exist yet: the contiguous, aligned fp32 [n, 128] output of a Linear."""
    dtype = torch.float32

    def __init__(self, n: int):
        self.shape = (int(n), 128)

    def dim(self):
        return 2

    def is_contiguous(self):
        return True

    def data_ptr(self):
        return 0

    def element_size(self):
        return 4

    def stride(self, i):
        return (128, 1)[i]


def takes_packed_epilogue(n_rows: int, inc: Incidence, norm: Optional[Tensor], aggr: str) -> bool:
    """Whether ``deepsets_aggregate(h, inc, norm, aggr, packed_rows=True)`` over the [n_rows, 128] fp32 output ``h`` of a Linear would
    gather packed rows, and the switch lets the Linear write them itself -- from the arguments alone (no data pass, no sync), BEFORE
    that Linear runs.  The caller adds the Linear's own conditions (``dense.fused_norm_linear_packed_supported``)."""
    if _PACKED_EPILOGUE == "off" or (_PACKED_EPILOGUE == "auto" and n_rows < PACKED_EPILOGUE_MIN_ROWS) or aggr not in REDUCE_CODES:
        return False
    # (a norm not yet known to be all ones -- its first sighting or two, Incidence.weights -- keeps the dense table for that forward)
    if not inc.known_unweighted(norm) or not (inc.src_extent <= n_rows <= inc.n_src):
        return False
    return _takes_packed(_RowsToCome(n_rows), None, inc, REDUCE_CODES[aggr])


def _takes_packed(x: Tensor, w_dst: Optional[Tensor], inc: Incidence, reduce: int) -> bool:
    """The packed path's conditions, from the arguments alone (no data pass, no sync: capturable): fp32, d = 128, contiguous
    16-byte aligned rows, SUM / MEAN without weights, one wave per row without a split tail."""
    if not (_PACKED_GATHER and x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == 128 and x.is_contiguous()
            and x.data_ptr() % 16 == 0 and reduce in (SUM, MEAN) and w_dst is None and x.shape[0] > 0 and inc.n_dst > 0):
        return False
    csr = inc.by_dst
    return _variant(csr, "segreduce", inc.n_dst, x) == 1 and not (0 < _split(csr, x) < inc.n_dst)


class _SegReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, w_dst: Optional[Tensor], w_src: Optional[Tensor], inc: Incidence, reduce: int, packed_rows: bool = False,
                packed: Optional[Tensor] = None, packed_fmt: Optional[str] = None):
        csr = inc.by_dst
        ext = reduce in (MAX, MIN)
        # ``packed`` came with ``x`` (dense.PackedRows): ``x`` is the overflow side table of a Linear that wrote the rows itself -- mostly
        # uninitialised, and read by the packed gather alone, for its overflow rows
        if packed is not None and not _takes_packed(x, w_dst, inc, reduce):
            raise _lib.AllSetHipError("deepsets_aggregate: packed rows came without a packed gather to read them "
                                      "(functional.takes_packed_epilogue decides the route before the Linear runs)")
        if packed is not None or (packed_rows and _takes_packed(x, w_dst, inc, reduce)):
            fmt = packed_fmt if packed is not None else packed_format()
            if packed is None:
                # the packed table is a temporary of this forward (the unweighted backward never reads the gathered table)
                packed = ops.pack_rows(x, fmt=fmt)
            out = ops.segreduce_packed(reduce, csr.rowptr, csr.col, packed, x, inc.n_dst, row_order=csr.row_order, fmt=fmt)
            arg = None
        else:
            out, arg = ops.segreduce(reduce, csr.rowptr, csr.col, w_dst, x, inc.n_dst, want_arg=ext,
                                     variant=1 if ext else _variant(csr, "segreduce", inc.n_dst, x), row_order=csr.row_order,
                                     split=_split(csr, x))
        need_gw = w_dst is not None and ctx.needs_input_grad[1]
        ctx.inc, ctx.reduce, ctx.n_s, ctx.need_gw = inc, reduce, x.shape[0], need_gw
        ctx.save_for_backward(x if need_gw else None, w_dst, w_src, arg)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout: Tensor):
        x, w_dst, w_src, arg = ctx.saved_tensors
        inc, reduce = ctx.inc, ctx.reduce
        T = inc.by_src
        gx = gw = None
        gout = gout.contiguous()
        if reduce in (MAX, MIN) or ctx.need_gw:
            if gout.dtype != torch.float32:
                raise _lib.AllSetHipError("max/min backward and weight gradients are fp32-only; bf16 storage covers "
                                          "sum/mean and the PMA path")
        if ctx.needs_input_grad[0]:
            if w_dst is not None and w_src is None:       # differentiable weights: route on the fly
                w_src = w_dst[inc.pos_dst_of_src().long()]
            if reduce in (SUM, MEAN):
                if reduce == MEAN:
                    inv = inc.inv_count_by_src()
                    w_src = inv if w_src is None else w_src * inv
                gx, _ = ops.segreduce(SUM, T.rowptr, T.col, w_src, gout, ctx.n_s,
                                      variant=_variant(T, "segreduce", ctx.n_s, gout), row_order=T.row_order,
                                      split=_split(T, gout) if ctx.n_s == T.n_rows else -1)
            else:
                gx = ops.segmax_bwd(T.rowptr, T.col, inc.pos_dst_of_src(), w_src, arg, gout, ctx.n_s)
        if ctx.need_gw:
            csr = inc.by_dst
            gw = ops.sddmm_rowdot(reduce, csr.rowptr, csr.col, x, gout, arg)
        return gx, gw, None, None, None, None, None, None


def deepsets_aggregate(x: Tensor, inc: Incidence, norm: Optional[Tensor] = None, aggr: str = "add",
                       packed_rows: bool = False) -> Tensor:
    """``out[t] = reduce_{i: dst_i = t} norm_i * x[src_i]`` for ``aggr`` in add|sum|mean|max|min.

    ``norm`` is per incidence in the caller's edge-list order (int64 ones in the reference default,
    preprocessing.py:454); ``None`` or all-ones skips the weight stream.  Output has ``inc.n_dst`` rows.
    ``packed_rows``: the caller's hint that ``x`` is mostly zeros (``dropout(relu(.))`` at p >= 0.5): where the packed gather is built
    (``_takes_packed``) the forward gathers packed nonzero rows; same result bit for bit, and a wrong hint is only slower.
    ``x`` may be a ``dense.PackedRows`` (a Linear that packed its own output, after ``takes_packed_epilogue``): gathered as it is.
    """
    if aggr not in REDUCE_CODES:
        raise ValueError(f"unknown aggr {aggr!r}")
    packed, packed_fmt = None, None
    if isinstance(x, PackedRows):
        x, packed, packed_fmt = x._side, x.packed, x.format
    _lib.require_device(x)
    _check_rows(x, inc)
    if norm is not None and norm.requires_grad:
        # differentiable routing (LearnMask): edge-list order -> the two CSR orders, ONCE per norm tensor and CSR -- every conv of a
        # forward gets the same ``Importance * norm`` object (models.py:451-452) and V->E / E->V share the two CSRs, so a two-layer
        # model routes twice per forward and twice per backward instead of three gathers per aggregation
        w_dst = _routed(norm, inc, True)
        w_src = _routed(norm, inc, False).detach()        # (only the input gradient reads it; the weight gradient flows through w_dst)
    else:
        w_dst, w_src = inc.weights(norm)
    return _SegReduce.apply(x, w_dst, w_src, inc, REDUCE_CODES[aggr], bool(packed_rows), packed, packed_fmt)


# ---- exclude-self Deep Sets aggregation over the UNEXPANDED incidence (csrc/loo.hip) ------------------------
def _loo_expand(x: Tensor, loo: LeaveOneOutIncidence, s_src: Optional[Tensor], s_seg: Optional[Tensor]) -> Tensor:
    """[rows of vertices] -> [nnz]: row (e, i) = s_seg[e] * sum of the scaled rows of e's members other than the i-th."""
    return ops.loo_rows(loo.e_rowptr, loo.e_col, x, s_src, s_seg, long_seg=loo.long_seg if loo.n_long else None, n_long=loo.n_long)


def _loo_collect(y: Tensor, loo: LeaveOneOutIncidence, s_seg: Optional[Tensor], w_inc: Optional[Tensor], n_rows: int) -> Tensor:
    """[nnz] -> [n_rows of vertices]: row v = sum over v's incidences (e, j) of w_inc * s_seg[e] * (sum of e's rows other than the j-th)."""
    t = ops.loo_rows(loo.e_rowptr, None, y, None, s_seg, long_seg=loo.long_seg if loo.n_long else None, n_long=loo.n_long)
    out, _ = ops.segreduce(SUM, loo.v_rowptr, loo.v_col, w_inc, t, n_rows)
    return out


class _LooV2E(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x: Tensor, loo: LeaveOneOutIncidence, f):
        ctx.loo, ctx.f, ctx.n_rows = loo, f, x.shape[0]
        return _loo_expand(x, loo, f.v2e_src, f.v2e_seg)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout: Tensor):
        f = ctx.f
        return _loo_collect(gout.contiguous(), ctx.loo, f.v2e_seg, f.v2e_src_inc, ctx.n_rows), None, None


class _LooE2V(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y: Tensor, loo: LeaveOneOutIncidence, f):
        ctx.loo, ctx.f = loo, f
        return _loo_collect(y, loo, f.e2v_seg, f.e2v_row_inc, loo.n_dst)

    @staticmethod
    @once_differentiable
    def backward(ctx, gout: Tensor):
        f = ctx.f
        return _loo_expand(gout.contiguous(), ctx.loo, f.e2v_row, f.e2v_seg), None, None


def deepsets_aggregate_exclude_self(x: Tensor, loo: LeaveOneOutIncidence, direction: str, aggr: str = "add",
                                    normtype: str = "all_one") -> Tensor:
    """``deepsets_aggregate`` over the reference's exclude-self expansion (``preprocessing.expand_edge_index``: hyperedge e of size k as
    k hyperedges ``e_i`` = e without its i-th member) computed from the UNEXPANDED incidence ``loo``:

    ``direction='v2e'``: ``x`` [n_v, d] -> [nnz, d], row (e, i) = reduce over the members of e other than the i-th;
    ``direction='e2v'``: ``x`` [nnz, d] -> [loo.n_dst, d], row v = reduce over every (e, i) with v in e and v not e's i-th member.

    ``aggr`` add | sum | mean (over the expanded sizes / degrees); ``normtype`` all_one | deg_half_sym (what ``norm_contruction`` gives on
    the expanded list).  A singleton hyperedge keeps its member, as in the reference.  Differentiable in ``x``; each direction's
    backward is the other's forward.  max / min, bf16 storage and a per-expanded-incidence weight (LearnMask) are not built here and
    raise ``NotImplementedError``: they keep the expansion path."""
    if direction not in ("v2e", "e2v"):
        raise ValueError(f"deepsets_aggregate_exclude_self: direction must be 'v2e' or 'e2v', got {direction!r}")
    f = loo.factors(aggr, normtype)
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise NotImplementedError(f"exclude-self aggregation: float32 only (got {x.dtype}); bf16 storage keeps the expansion path "
                                  "(preprocessing.expand_edge_index)")
    if direction == "v2e":
        if not (loo.n_dst <= x.shape[0] <= loo.n_v):
            raise ValueError(f"vertex matrix has {x.shape[0]} rows; the incidence needs between {loo.n_dst} and {loo.n_v}")
        return _LooV2E.apply(x, loo, f)
    if x.shape[0] != loo.nnz:
        raise ValueError(f"hyperedge-side matrix has {x.shape[0]} rows; the exclude-self incidence has {loo.nnz} (one per incidence)")
    return _LooE2V.apply(x, loo, f)


def _colocate(V: Tensor, heads: int) -> bool:
    """Feature rows of at most half a cache line (the column-sharded layer's d/P slices): put the per-row scalars the
    kernels gather -- logits forward, (M, delta) backward -- into the same 128-byte line as the row, so an incidence
    costs one cache-line request instead of two (profiles/r01_colshard_kernels.txt)."""
    row = V.shape[1] * V.element_size()
    return V.is_cuda and row % 16 == 0 and row + 8 * heads <= 128 and row <= 64 and V.shape[0] >= 4096


def _beside(rows: Tensor, small_cols: int) -> Tuple[Tensor, Tensor]:
    """A 128-byte-pitched buffer holding a copy of ``rows`` [n, d] and room for ``small_cols`` float32 per row behind it.
    Returns (view of the row copy [n, d], float32 view [n, small_cols]) -- both row-strided views of the one buffer."""
    n, d = rows.shape
    rb = d * rows.element_size()
    buf = torch.empty((n, 128), dtype=torch.uint8, device=rows.device)
    rv = buf[:, :rb].view(rows.dtype)
    rv.copy_(rows)
    return rv, buf[:, rb:rb + 4 * small_cols].view(torch.float32)


class _PmaAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, V: Tensor, alpha: Tensor, inc: Incidence, heads: int, slope: float):
        csr = inc.by_dst
        split = _split(csr, V, heads)
        Vg, ag = V, alpha
        if _colocate(V, heads) and split <= 0:
            Vg, ag = _beside(V, heads)
            ag.copy_(alpha)
        out, m, l = ops.pma_fwd(csr.rowptr, csr.col, ag, Vg, heads, slope, inc.n_dst,
                                variant=_variant(csr, "pma_fwd", inc.n_dst, V, heads), row_order=csr.row_order,
                                split=split, sizes=_sizes(csr, V, heads) if split <= 0 else None)
        ctx.inc, ctx.slope = inc, slope
        ctx.save_for_backward(V, alpha, out, m, l)
        ctx.mark_non_differentiable(m, l)
        ctx.set_materialize_grads(False)     # (m, l never carry a gradient: no [n, H] zero-fills for them in every backward)
        return out, m, l

    @staticmethod
    @once_differentiable
    def backward(ctx, gout: Tensor, _gm, _gl):
        if gout is None:
            return None, None, None, None, None
        V, alpha, out, m, l = ctx.saved_tensors
        T = ctx.inc.by_src
        gout = gout.contiguous()
        H = alpha.shape[1]
        split = _split(T, V, H)
        if _colocate(gout, H) and split <= 0:
            gout, sv = _beside(gout, 2 * H)
            stats = ops.pma_bwd_stats(out, gout, m, l, stats=sv.unflatten(1, (H, 2)))
        else:
            stats = ops.pma_bwd_stats(out, gout, m, l)
        gV, galpha = ops.pma_bwd_src(T.rowptr, T.col, alpha, V, gout, stats, ctx.slope,
                                     variant=_variant(T, "pma_bwd_src", V.shape[0], V, H),
                                     row_order=T.row_order, split=split, sizes=_sizes(T, V, H) if split <= 0 else None)
        return gV, galpha, None, None, None


class _PmaPoolLn0(torch.autograd.Function):
    """``LayerNorm_{gamma,beta}( pma_pool(V, alpha) + att_r )`` -- the pooling and the first LayerNorm of the PMA tail
    (reference layers.py:145-154) as ONE autograd node, so that the backward statistics of the pooling
    (``{m + log l, <out, gout>}`` per target and head) are written by the LayerNorm-backward kernel that already holds ``out``
    and its gradient in registers, instead of by a separate pass over both (allset_pma_bwd_stats: 0.22 ms per direction at 1M x 128)."""

    @staticmethod
    def forward(ctx, V, alpha, inc, heads, slope, att_r, gamma, beta, eps):
        from . import dense
        csr = inc.by_dst
        pooled, m, l = ops.pma_fwd(csr.rowptr, csr.col, alpha, V, heads, slope, inc.n_dst,
                                   variant=_variant(csr, "pma_fwd", inc.n_dst, V, heads), row_order=csr.row_order,
                                   split=_split(csr, V, heads), sizes=_sizes(csr, V, heads))
        cb = att_r.reshape(-1)
        y, stats = dense.ln_res_fwd(pooled, cb, None, gamma, beta, eps, False, 0.0, 0, None)
        ctx.inc, ctx.slope, ctx.cshape = inc, slope, att_r.shape
        ctx.params = {"gamma": gamma, "beta": beta, "colb": att_r}           # (the objects themselves: dense.deferred_param_grads assigns their .grad)
        ctx.save_for_backward(V, alpha, pooled, m, l, cb, stats, gamma, beta)
        ctx.mark_non_differentiable(m, l)
        ctx.set_materialize_grads(False)     # (m, l never carry a gradient: no [n, H] zero-fills for them in every backward)
        return y, m, l

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gm, _gl):
        from . import dense
        if gy is None:
            return (None,) * 9
        V, alpha, pooled, m, l, cb, stats, gamma, beta = ctx.saved_tensors
        g_pooled, dg, db, dc, pstats = dense.ln_res_bwd_pma(gy.contiguous(), pooled, cb, stats, gamma, beta, m, l,
                                                            params=dense._queue_params(ctx, {"colb": 5, "gamma": 6, "beta": 7}))
        T = ctx.inc.by_src
        H = alpha.shape[1]
        gV, galpha = ops.pma_bwd_src(T.rowptr, T.col, alpha, V, g_pooled, pstats, ctx.slope,
                                     variant=_variant(T, "pma_bwd_src", V.shape[0], V, H), row_order=T.row_order,
                                     split=_split(T, V, H), sizes=_sizes(T, V, H))
        return gV, galpha, None, None, None, (dc.reshape(ctx.cshape) if dc is not None else None), dg, db, None


_POOL_TAIL_INPUTS = dict(att_r=5, g0=6, b0=7, w1=9, b1=10, w2=11, b2=12, g1=13, bt1=14)      # (positions in _PmaPoolTail.forward)


class _PmaPoolTail(torch.autograd.Function):
    """Pooling + the whole PMA tail (reference layers.py:145-157) as ONE autograd node: ``pma_fwd`` and the two tail kernels of
    ``dense.pma_tail_fwd`` forward; backward as ``_PmaPoolLn0`` (the pooling's backward statistics come out of ln0's backward
    pass) with ln1's backward reading the saved sum."""

    @staticmethod
    def forward(ctx, V, alpha, inc, heads, slope, att_r, g0, b0, eps0, w1, b1, w2, b2, g1, bt1, eps1, relu_post, p):
        from . import dense
        csr = inc.by_dst
        pooled, m, l = ops.pma_fwd(csr.rowptr, csr.col, alpha, V, heads, slope, inc.n_dst,
                                   variant=_variant(csr, "pma_fwd", inc.n_dst, V, heads), row_order=csr.row_order,
                                   split=_split(csr, V, heads), sizes=_sizes(csr, V, heads))
        y, saved, cfg = dense.pma_tail_fwd(pooled, att_r.reshape(-1), g0, b0, eps0, w1, b1, w2, b2, g1, bt1, eps1, relu_post, p)
        ctx.inc, ctx.slope, ctx.cshape, ctx.cfg = inc, slope, att_r.shape, cfg
        ctx.params = dict(att_r=att_r, g0=g0, b0=b0, w1=w1, b1=b1, w2=w2, b2=b2, g1=g1, bt1=bt1)     # (the objects themselves: dense.deferred_param_grads assigns their .grad)
        ctx.save_for_backward(V, alpha, m, l, *saved)
        ctx.mark_non_differentiable(m, l)
        ctx.set_materialize_grads(False)     # (m, l never carry a gradient: no [n, H] zero-fills for them in every backward)
        return y, m, l

    @staticmethod
    @once_differentiable
    def backward(ctx, gy, _gm, _gl):
        from . import dense
        if gy is None:
            return (None,) * 18
        V, alpha, m, l = ctx.saved_tensors[:4]
        g_pooled, dc, dg0, db0, gw1, gb1, gw2, gb2, dg1, db1, pstats = dense.pma_tail_bwd(
            ctx.saved_tensors[4:], ctx.cfg, gy, m, l, params=dense._queue_params(ctx, _POOL_TAIL_INPUTS))
        T = ctx.inc.by_src
        H = alpha.shape[1]
        gV, galpha = ops.pma_bwd_src(T.rowptr, T.col, alpha, V, g_pooled, pstats, ctx.slope,
                                     variant=_variant(T, "pma_bwd_src", V.shape[0], V, H), row_order=T.row_order,
                                     split=_split(T, V, H), sizes=_sizes(T, V, H))
        return (gV, galpha, None, None, None, (dc.reshape(ctx.cshape) if dc is not None else None), dg0, db0, None, gw1, gb1, gw2, gb2,
                dg1, db1, None, None, None)


def pma_pool_tail(V: Tensor, alpha: Tensor, inc: Incidence, heads: int, negative_slope: float, att_r: Tensor, g0, b0, eps0, w1, b1, w2, b2,
                  g1, bt1, eps1, relu_post: bool, p: float) -> Tuple[Tensor, Tensor, Tensor]:
    """``(tail(pool(V, alpha)), m, l)``; see :class:`_PmaPoolTail` (callers check ``pma_pool_ln0_supported`` and
    ``dense.pma_tail_supported``)."""
    _lib.require_device(V, alpha)
    _check_rows(V, inc)
    if alpha.dtype != torch.float32:
        alpha = alpha.float()
    return _PmaPoolTail.apply(V, alpha, inc, int(heads), float(negative_slope), att_r, g0, b0, float(eps0), w1, b1, w2, b2, g1, bt1,
                              float(eps1), bool(relu_post), float(p))


def pma_pool_ln0_supported(V: Tensor, heads: int) -> bool:
    from . import dense
    d = V.shape[1]
    return (V.is_cuda and V.dtype in (torch.float32, torch.bfloat16) and dense.ln_res_supported(d, V.dtype)
            and dense.ln_res_bwd_pma_supported(d, heads, V.dtype) and not _colocate(V, heads))


def pma_pool_ln0(V: Tensor, alpha: Tensor, inc: Incidence, heads: int, negative_slope: float, att_r: Tensor, gamma: Tensor,
                 beta: Tensor, eps: float) -> Tuple[Tensor, Tensor, Tensor]:
    """``(LayerNorm(pool(V, alpha) + att_r), m, l)``; see :class:`_PmaPoolLn0`."""
    _lib.require_device(V, alpha)
    _check_rows(V, inc)
    if alpha.dtype != torch.float32:
        alpha = alpha.float()
    return _PmaPoolLn0.apply(V, alpha, inc, int(heads), float(negative_slope), att_r, gamma, beta, float(eps))


def pma_aggregate(V: Tensor, alpha: Tensor, inc: Incidence, heads: int, negative_slope: float = 0.2
                  ) -> Tuple[Tensor, Tensor, Tensor]:
    """Softmax-attention pooling: ``out[t,h,:] = sum_i softmax_i(leaky_relu(alpha[src_i,h])) * V[src_i,h,:]``.

    ``V``: [n_src, heads*C], ``alpha``: [n_src, heads] (pre-activation).  Returns
    ``(out [n_dst, heads*C], m [n_dst, heads], l [n_dst, heads])``; empty targets give 0.
    """
    _lib.require_device(V, alpha)
    _check_rows(V, inc)
    if alpha.dtype != torch.float32:          # logits and softmax statistics are always fp32 (bf16 is storage only)
        alpha = alpha.float()
    return _PmaAggregate.apply(V, alpha, inc, int(heads), float(negative_slope))


def pma_attention_weights(alpha: Tensor, m: Tensor, l: Tensor, inc: Incidence, negative_slope: float = 0.2) -> Tensor:
    """Per-incidence attention weights [nnz, heads] in the caller's edge-list order
    (reference ``PMA.forward(..., return_attention_weights=True)``, layers.py:159-162)."""
    csr = inc.by_dst
    p_csr = ops.pma_attention(csr.rowptr, csr.col, alpha.detach(), m, l, float(negative_slope))
    p = torch.empty_like(p_csr)
    p[csr.perm.long()] = p_csr
    return p


# ---- exclude-self PMA pooling over the UNEXPANDED incidence (csrc/loo_softmax.hip) ----------------------------
def _loo_long(loo: LeaveOneOutIncidence) -> dict:
    return dict(long_seg=loo.long_seg if loo.n_long else None, n_long=loo.n_long)


class _LooSoftmaxV2E(torch.autograd.Function):
    """[vertices] -> [nnz]: row (e, i) = the softmax pooling of e's members other than the i-th.  Backward: the per-position gradients
    of the leave-one-out softmax, summed per vertex by ``segreduce`` over the vertex-major CSR (as ``_loo_collect`` does)."""

    @staticmethod
    def forward(ctx, V: Tensor, alpha: Tensor, loo: LeaveOneOutIncidence, heads: int, slope: float):
        out, lse = ops.loo_softmax_fwd(loo.e_rowptr, loo.e_col, alpha, V, heads, slope, **_loo_long(loo))
        ctx.loo, ctx.heads, ctx.slope = loo, heads, slope
        ctx.save_for_backward(V, alpha, out, lse)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout: Tensor):
        V, alpha, out, lse = ctx.saved_tensors
        loo = ctx.loo
        gV_pos, ga_pos = ops.loo_softmax_bwd(loo.e_rowptr, loo.e_col, alpha, V, ctx.heads, ctx.slope, out, lse, gout.contiguous(), None,
                                             **_loo_long(loo))
        gV, _ = ops.segreduce(SUM, loo.v_rowptr, loo.v_col, None, gV_pos, V.shape[0])
        galpha, _ = ops.segreduce(SUM, loo.v_rowptr, loo.v_col, None, ga_pos, V.shape[0])
        return gV, galpha, None, None, None


class _LooSoftmaxStates(torch.autograd.Function):
    """Stage 1 of E->V: the nnz contiguous hyperedge-side rows -> per position the normalised softmax state ``(o, L)`` of "every row of
    its hyperedge but its own".  Takes both cotangents (stage 2, the ordinary pooling with logits ``L``, supplies them)."""

    @staticmethod
    def forward(ctx, V: Tensor, alpha: Tensor, loo: LeaveOneOutIncidence, heads: int, slope: float):
        out, lse = ops.loo_softmax_fwd(loo.e_rowptr, None, alpha, V, heads, slope, **_loo_long(loo))
        ctx.loo, ctx.heads, ctx.slope = loo, heads, slope
        ctx.save_for_backward(V, alpha, out, lse)
        ctx.set_materialize_grads(False)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, gout: Optional[Tensor], glse: Optional[Tensor]):
        if gout is None and glse is None:
            return None, None, None, None, None
        V, alpha, out, lse = ctx.saved_tensors
        loo = ctx.loo
        gout = torch.zeros_like(out) if gout is None else gout.contiguous()
        gV, galpha = ops.loo_softmax_bwd(loo.e_rowptr, None, alpha, V, ctx.heads, ctx.slope, out, lse, gout,
                                         glse.contiguous() if glse is not None else None, **_loo_long(loo))
        return gV, galpha, None, None, None


def pma_exclude_self_states(V: Tensor, alpha: Tensor, loo: LeaveOneOutIncidence, heads: int, negative_slope: float = 0.2
                            ) -> Tuple[Tensor, Tensor]:
    """Stage 1 of the exclude-self E->V pooling: ``V`` [nnz, heads*C], ``alpha`` [nnz, heads] (the hyperedge-side rows, one per
    incidence) -> ``(o [nnz, heads*C], L [nnz, heads])``, per position the softmax pooling of the OTHER rows of its hyperedge and the
    log of its normaliser.  Pooling ``o`` with logits ``L`` (slope 1) over ``loo.merge_incidence()`` completes the direction."""
    _check_exclude_self_pma(V, alpha, heads)
    if V.shape[0] != loo.nnz:
        raise ValueError(f"hyperedge-side matrix has {V.shape[0]} rows; the exclude-self incidence has {loo.nnz} (one per incidence)")
    return _LooSoftmaxStates.apply(V, alpha, loo, int(heads), float(negative_slope))


def _check_exclude_self_pma(V: Tensor, alpha: Tensor, heads: int) -> None:
    _lib.require_device(V, alpha)
    if V.dtype != torch.float32 or alpha.dtype != torch.float32:
        raise NotImplementedError(f"exclude-self PMA pooling: float32 only (got V {V.dtype}, alpha {alpha.dtype}); bf16 storage keeps the "
                                  "expansion path (preprocessing.expand_edge_index)")
    if V.dim() != 2 or alpha.dim() != 2 or alpha.shape[0] != V.shape[0] or alpha.shape[1] != heads:
        raise ValueError(f"V must be [n, heads*C] and alpha [n, heads]; got {tuple(V.shape)} and {tuple(alpha.shape)} for {heads} heads")
    if not ops.loo_softmax_supported(V.shape[1], heads):
        raise _lib.AllSetHipError(f"exclude-self PMA pooling: d = {V.shape[1]} with {heads} heads is not built (heads 1 | 2 | 4 | 8, "
                                  "(d / heads) % 4 == 0, d <= 512); expand the edge list with preprocessing.expand_edge_index instead")


def pma_aggregate_exclude_self(V: Tensor, alpha: Tensor, loo: LeaveOneOutIncidence, direction: str, heads: int,
                               negative_slope: float = 0.2) -> Tensor:
    """``pma_aggregate`` over the reference's exclude-self expansion (``preprocessing.expand_edge_index``) computed from the UNEXPANDED
    incidence ``loo`` (a leave-one-out softmax):

    ``direction='v2e'``: ``V`` [n_v, heads*C], ``alpha`` [n_v, heads] -> [nnz, heads*C], row (e, i) = the pooling of e's members other
    than the i-th;
    ``direction='e2v'``: ``V`` [nnz, heads*C], ``alpha`` [nnz, heads] -> [loo.n_dst, heads*C], row v = the pooling of every (e, i) with v
    in e and v not e's i-th member: per hyperedge the state of "all rows but v's own", then the merge of v's states (``pma_aggregate``
    with the states' log-normalisers as logits).

    A singleton hyperedge keeps its member, as in the reference.  Differentiable in ``V`` and ``alpha``.  fp32, heads 1 | 2 | 4 | 8,
    C % 4 == 0, d <= 512; anything else raises (bf16 storage and LearnMask keep the expansion path)."""
    if direction not in ("v2e", "e2v"):
        raise ValueError(f"pma_aggregate_exclude_self: direction must be 'v2e' or 'e2v', got {direction!r}")
    if direction == "v2e":
        _check_exclude_self_pma(V, alpha, heads)
        if not (loo.n_dst <= V.shape[0] <= loo.n_v):
            raise ValueError(f"vertex matrix has {V.shape[0]} rows; the incidence needs between {loo.n_dst} and {loo.n_v}")
        return _LooSoftmaxV2E.apply(V, alpha, loo, int(heads), float(negative_slope))
    o, L = pma_exclude_self_states(V, alpha, loo, heads, negative_slope)
    out, _, _ = pma_aggregate(o, L, loo.merge_incidence(), heads, 1.0)
    return out


# ---- degree-scaled propagate of the hypergraph-convolution baselines (HCHA / HGNN / HNHN; csrc/hconv.hip) ----------------------
def _epilogue_backward(gy, y, act, p, seed, base, epi, bias=None, need_b=False):
    """Backward of a hop's row epilogue ``y = drop_p(act(v + bias))``: ``(g, gb)``, the gradients of ``v`` and -- with ``need_b`` -- of
    the bias.  Without an epilogue ``gy`` passes through."""
    if not epi:
        return gy, None
    from . import dense
    g, part = ops.hconv_bwd_epi(gy, y, act, p, seed, base, want_bias=need_b)
    gb = None
    if need_b:
        # (inside dense.deferred_param_grads(): queued for the step's one batched reduction, and None here)
        (gb,) = dense._finish_partials(part, [("bias", 0, (y.shape[1],))], {"bias": bias})
    return g, gb


class _ScaledPropagate(torch.autograd.Function):
    """``y = drop_p(act(s * (H^T or H)(r * x) + bias))`` -- one kernel forward; backward: the epilogue's kernel (only when there is
    an epilogue) and the same propagate kernel over the opposite CSR with ``r`` and ``s`` swapped.  ``r`` / ``s`` are constants."""

    @staticmethod
    def forward(ctx, x, bias, inc, to_dst, r, s, act, p, variant):
        from . import dense
        fwd, bwd = (inc.by_dst, inc.by_src) if to_dst else (inc.by_src, inc.by_dst)
        n_t, n_s = (inc.n_dst, inc.n_src) if to_dst else (inc.n_src, inc.n_dst)
        if x.shape[0] != n_s:
            raise _lib.AllSetHipError(f"scaled_propagate: x has {x.shape[0]} rows, the incidence gathers from {n_s}")
        seed, base = dense._seed_for(p)
        y = ops.hconv_propagate(fwd, x, n_t, r, s, bias, act, p, seed, base, variant)
        epi = act is not None or p > 0.0 or bias is not None
        ctx.save_for_backward(y if epi else None)
        ctx.cfg = (bwd, n_s, r, s, act, p, seed, base, epi, variant)
        ctx.bias_param = bias
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        bwd, n_s, r, s, act, p, seed, base, epi, variant = ctx.cfg
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[1]
        g, gb = _epilogue_backward(gy, y, act, p, seed, base, epi, ctx.bias_param, need_b)
        gx = ops.hconv_propagate(bwd, g, n_s, r=s, s=r, variant=variant) if ctx.needs_input_grad[0] else None
        return gx, gb, None, None, None, None, None, None, None


class _WeightedPropagate(torch.autograd.Function):
    """``y = drop_p(act(A_w x + bias))`` over the target-major CSR with the per-incidence weights ``w_dst`` -- one kernel forward;
    backward: the epilogue's kernel (only when there is an epilogue) and the same kernel over the source-major CSR with the weights
    in that CSR's order, ``w_src``.  The weights are constants."""

    @staticmethod
    def forward(ctx, x, bias, inc, w_dst, w_src, act, p, variant):
        from . import dense
        if x.shape[0] != inc.n_src:
            raise _lib.AllSetHipError(f"weighted_propagate: x has {x.shape[0]} rows, the graph gathers from {inc.n_src}")
        seed, base = dense._seed_for(p)
        y = ops.hconv_propagate_w(inc.by_dst, x, inc.n_dst, w_dst, bias, act, p, seed, base, variant)
        epi = act is not None or p > 0.0 or bias is not None
        ctx.save_for_backward(y if epi else None)
        ctx.cfg = (inc, w_src, act, p, seed, base, epi, variant)
        ctx.bias_param = bias
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        inc, w_src, act, p, seed, base, epi, variant = ctx.cfg
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[1]
        g, gb = _epilogue_backward(gy, y, act, p, seed, base, epi, ctx.bias_param, need_b)
        gx = ops.hconv_propagate_w(inc.by_src, g, inc.n_src, w_src, variant=variant) if ctx.needs_input_grad[0] else None
        return gx, gb, None, None, None, None, None, None


def weighted_propagate(x: Tensor, inc: Incidence, w_dst: Optional[Tensor], w_src: Optional[Tensor], bias: Optional[Tensor] = None,
                       act: Optional[str] = None, p: float = 0.0, variant: Optional[int] = None) -> Tensor:
    """One GCN hop (PyG ``GCNConv.propagate`` with ``edge_weight``): ``y[t] = drop_p(act(sum_{edges s -> t} w_e * x[s] + bias))``
    over ``inc`` (sources -> targets; ``inc.n_dst`` output rows).  ``w_dst`` / ``w_src``: the edge weights routed into
    ``inc.by_dst`` / ``inc.by_src`` order (both None = ones).  ``act`` None / 'relu' / 'elu'; ``p`` the dropout probability.
    Differentiable in ``x`` and ``bias``.  ``variant``: kernel variant override of the forward and the backward launch (tests)."""
    if act not in ops.HCONV_ACTS:
        raise ValueError(f"weighted_propagate: act must be None, 'relu' or 'elu', got {act!r}")
    if (w_dst is None) != (w_src is None):
        raise ValueError("weighted_propagate: give the weights in both CSR orders, or neither")
    return _WeightedPropagate.apply(x, bias, inc, w_dst, w_src, act, float(p), variant)


class _CliquePropagate(torch.autograd.Function):
    """The GCN hop over the clique expansion from prefix sums over the hyperedges (``graph``: a ``baselines.ImplicitCEGraph``).  Forward:
    ``ops.scan_rows`` (exclusive prefix of ``dinv * x`` inside every hyperedge) and ``ops.scan_collect`` (sum over a vertex's positions,
    the self-loop term, ``dinv``, the row epilogue).  Backward: the epilogue's kernel (only when there is an epilogue), then the same two
    launches with the exclusive SUFFIX.  ``x`` arrives padded to a multiple of 4 columns; ``width`` is the logical width."""

    @staticmethod
    def forward(ctx, x, bias, graph, act, p, width):
        from . import dense
        seed, base = dense._seed_for(p)
        long = dict(long_seg=graph.long_seg if graph.n_long else None, n_long=graph.n_long)
        t = ops.scan_rows(graph.e_rowptr, graph.e_col, x, graph.dinv, reverse=False, **long)
        y = ops.scan_collect(graph.v_rowptr, graph.v_pos, t, x, graph.r_self, graph.dinv, bias, act, p, seed, base, width=width)
        y = y if width == y.shape[1] else y[:, :width]
        epi = act is not None or p > 0.0 or bias is not None
        ctx.save_for_backward(y if epi else None)
        ctx.cfg = (graph, long, act, p, seed, base, epi, x.shape[1])
        ctx.bias_param = bias
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        graph, long, act, p, seed, base, epi, d = ctx.cfg
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[1]
        g, gb = _epilogue_backward(gy, y, act, p, seed, base, epi, ctx.bias_param, need_b)
        gx = None
        if ctx.needs_input_grad[0]:
            g = _pad_columns(g, d)
            t = ops.scan_rows(graph.e_rowptr, graph.e_col, g, graph.dinv, reverse=True, **long)
            gx = ops.scan_collect(graph.v_rowptr, graph.v_pos, t, g, graph.r_self, graph.dinv)
        return gx, gb, None, None, None, None


def _pad_columns(x: Tensor, d: int) -> Tensor:
    return x if x.shape[1] == d else torch.nn.functional.pad(x, (0, d - x.shape[1]))


def clique_propagate(x: Tensor, graph, bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0) -> Tensor:
    """One GCN hop over the clique expansion of a hypergraph WITHOUT the expansion: what
    ``weighted_propagate`` computes over ``ConstructV2V`` + ``norm_contruction(TYPE='V2V')``,

    ``y[j] = drop_p(act(dinv[j] * (sum_{e ni j} sum_{i in e, i < j} dinv[i] * x[i] + loop[j] * dinv[j] * x[j]) + bias))``,

    from ``graph`` (a ``baselines.ImplicitCEGraph``): O(nnz * C) traffic, O(nnz) index memory.  ``act`` None / 'relu' / 'elu'; ``p`` the
    dropout probability.  Differentiable in ``x`` and ``bias``.  fp32, any width 1 <= C <= 512 (a width that is no multiple of 4 is
    padded with zero columns around the two launches); anything else raises -- there is no fallback."""
    if act not in ops.HCONV_ACTS:
        raise ValueError(f"clique_propagate: act must be None, 'relu' or 'elu', got {act!r}")
    _lib.require_device(x, bias)
    if x.dtype != torch.float32:
        raise NotImplementedError(f"clique_propagate: float32 only (got {x.dtype}); bf16 storage is not built -- use the explicit "
                                  "expansion (preprocessing.ConstructV2V)")
    if x.dim() != 2 or x.shape[0] != graph.n:
        raise _lib.AllSetHipError(f"clique_propagate: x is {tuple(x.shape)}, the graph has {graph.n} vertex rows")
    C = x.shape[1]
    if not 1 <= C <= 512:
        raise _lib.AllSetHipError(f"clique_propagate: width {C} is not built (1 <= C <= 512); there is no fallback -- use the explicit "
                                  "expansion (preprocessing.ConstructV2V)")
    if bias is not None and bias.numel() != C:
        raise _lib.AllSetHipError(f"clique_propagate: bias has {bias.numel()} entries for width {C}")
    return _CliquePropagate.apply(_pad_columns(x, (C + 3) // 4 * 4), bias, graph, act, float(p), C)


def scaled_propagate(x: Tensor, inc: Incidence, direction: str, r: Optional[Tensor] = None, s: Optional[Tensor] = None,
                     bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0, variant: Optional[int] = None) -> Tensor:
    """One hop of a hypergraph convolution over ``inc`` (sources = vertices, targets = hyperedges):
    ``direction`` 'v2e': ``y[e] = drop_p(act(s[e] * sum_{v in e} r[v] * x[v] + bias))``;
    'e2v': ``y[v] = drop_p(act(s[v] * sum_{e ni v} r[e] * x[e] + bias))``.
    ``r`` (per gathered row), ``s`` (per output row) and ``bias`` may be None; ``act`` None / 'relu' / 'elu'; ``p`` the dropout
    probability (0 outside training).  Differentiable in ``x`` and ``bias``.  ``variant``: kernel variant override of the forward
    and the backward launch (tests)."""
    if direction not in ("v2e", "e2v"):
        raise ValueError(f"scaled_propagate: direction must be 'v2e' or 'e2v', got {direction!r}")
    if act not in ops.HCONV_ACTS:
        raise ValueError(f"scaled_propagate: act must be None, 'relu' or 'elu', got {act!r}")
    return _ScaledPropagate.apply(x, bias, inc, direction == "v2e", r, s, act, float(p), variant)


# ---- GAT attention hop of the clique-expansion baseline CEGAT (csrc/gat.hip) ----------------------------------------------------
class _GatPropagate(torch.autograd.Function):
    """``y = drop_p(act(concat_h or mean_h softmax_j(lrelu(al[s_j] + ar[t])) x[s_j] + bias))`` -- one kernel forward.  Backward:
    the epilogue's kernel (only when there is an epilogue), one pass over the target rows for the softmax statistics and the whole
    of ``gar``, one gather pass over the source-major CSR for ``gx`` and ``gal``.  Saved: ``x``, ``al``, ``ar``, ``y``, the
    positive-logit part of the aggregate (``aggpos`` [n, H*C], ``ppos`` [n, H]), ``m``, ``l``, and -- head-mean form only -- the
    aggregate itself (the concat form rebuilds it from ``y``, ``bias`` and the mask)."""

    @staticmethod
    def forward(ctx, x, al, ar, bias, inc, heads, slope, concat, act, p):
        from . import dense
        if x.shape[0] != inc.n_src:
            raise _lib.AllSetHipError(f"gat_propagate: x has {x.shape[0]} rows, the graph gathers from {inc.n_src}")
        seed, base = dense._seed_for(p)
        want = any(ctx.needs_input_grad[:4])
        y, agg, aggpos, ppos, m, l = ops.gat_fwd(inc.by_dst, x, al, ar, heads, slope, inc.n_dst, concat, bias, act, p, seed, base,
                                                 want_grad=want)
        epi = act is not None or p > 0.0 or bias is not None
        ctx.save_for_backward(x, al, ar, y if (epi or concat) else None, agg, aggpos, ppos, m, l)
        ctx.cfg = (inc, heads, slope, concat, act, p, seed, base, epi)
        ctx.bias_param = bias
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, al, ar, y, agg, aggpos, ppos, m, l = ctx.saved_tensors
        inc, heads, slope, concat, act, p, seed, base, epi = ctx.cfg
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[3]
        g, gb = _epilogue_backward(gy, y, act, p, seed, base, epi, ctx.bias_param, need_b)
        if concat:
            stats, gar = ops.gat_bwd_stats(g, aggpos, ppos, m, l, slope, y=y, bias=ctx.bias_param, p=p)
        else:
            g = (g * (1.0 / heads)).repeat(1, heads)                   # the head mean's backward: g / H to every head
            stats, gar = ops.gat_bwd_stats(g, aggpos, ppos, m, l, slope, agg=agg)
        gx, gal = ops.gat_bwd_src(inc.by_src, x, al, ar, g, stats, slope)
        return gx, gal, gar, gb, None, None, None, None, None, None


def gat_propagate(x: Tensor, al: Tensor, ar: Tensor, inc: Incidence, heads: int, negative_slope: float = 0.2, concat: bool = True,
                  bias: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0) -> Tensor:
    """One GAT hop (torch_geometric 1.6.3 ``GATConv.propagate`` + bias, without attention dropout) over ``inc`` (sources -> targets;
    ``inc.n_dst`` output rows): with ``e_j = leaky_relu(al[s_j, h] + ar[t, h])`` and ``p_j`` its softmax over the edges into ``t``,
    ``agg[t, h] = sum_j p_j x[s_j, h]``; ``y = drop_p(act(agg + bias))`` with the heads side by side (``concat``) or averaged.
    ``x`` [n_src, heads * C], ``al`` [n_src, heads], ``ar`` [n_dst, heads]; ``act`` None / 'relu'; ``p`` the dropout probability on
    the OUTPUT (the library's hash mask).  Differentiable in ``x``, ``al``, ``ar`` and ``bias``."""
    if act not in ops.RELU_ACTS:
        raise ValueError(f"gat_propagate: act must be None or 'relu', got {act!r}")
    _lib.require_device(x, al, ar)
    if al.dtype != torch.float32 or ar.dtype != torch.float32:
        al, ar = al.float(), ar.float()
    return _GatPropagate.apply(x, al, ar, bias, inc, int(heads), float(negative_slope), bool(concat), act, float(p))


# ---- hypergraph attention of HCHA's HypergraphConv(use_attention=True) (csrc/hattn.hip) --------------------------------------------
class _HattnPropagate(torch.autograd.Function):
    """Both hops of the attention conv under one coefficient: the coefficient launch (vertex-major softmax + coefficient dropout,
    written in both CSR orders), the V->E hop, the E->V hop with the epilogue.  Backward: the epilogue's kernel (only when there is an
    epilogue), the E->V hop's transpose over the hyperedge-major CSR, one vertex-major gather pass (the V->E hop's transpose, ``gav`` and
    the per-incidence logit gradient), one segment sum for ``gae``.  Saved: ``z``, ``av``, ``ae``, the coefficients in both orders
    ([nnz, H] each), ``m``, ``l``, the V->E hop's output and, with an epilogue, the output."""

    @staticmethod
    def forward(ctx, z, av, ae, bias, inc, heads, D, B, slope, concat, act, p_attn, p):
        from . import dense
        n_v, n_e = inc.n_src, inc.n_dst
        if z.shape[0] != n_v or tuple(av.shape) != (n_v, heads) or tuple(ae.shape) != (n_e, heads):
            raise _lib.AllSetHipError(f"hattn_propagate: z {tuple(z.shape)} / av {tuple(av.shape)} / ae {tuple(ae.shape)} against "
                                      f"{n_v} vertices, {n_e} hyperedges and {heads} heads")
        if D.numel() != n_v or B.numel() != n_e:
            raise _lib.AllSetHipError(f"hattn_propagate: D has {D.numel()} entries for {n_v} vertices, B {B.numel()} for {n_e} hyperedges")
        seed_a, base_a = dense._seed_for(p_attn)                     # (drawn first: the coefficient's mask, then the output's)
        seed, base = dense._seed_for(p)
        pos = inc.pos_dst_of_src()
        a_v, a_e, m, l = ops.hattn_coef(inc.by_src, pos, av, ae, slope, p_attn, seed_a, base_a)
        y_e = ops.hattn_hop(inc.by_dst, a_e, z, heads, n_e, s=B)
        out = ops.hattn_hop(inc.by_src, a_v, y_e, heads, n_v, s=D, concat=concat, bias=bias, act=act, p=p, seed=seed, seed_base=base)
        epi = act is not None or p > 0.0 or bias is not None
        ctx.save_for_backward(z, av, ae, a_v, a_e, m, l, y_e, out if epi else None, D, B)
        ctx.cfg = (inc, heads, slope, concat, act, p, seed, base, epi)
        ctx.bias_param = bias
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        z, av, ae, a_v, a_e, m, l, y_e, out, D, B = ctx.saved_tensors
        inc, heads, slope, concat, act, p, seed, base, epi = ctx.cfg
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[3]
        g, gb = _epilogue_backward(gout, out, act, p, seed, base, epi, ctx.bias_param, need_b)
        if not concat:
            g = (g * (1.0 / heads)).repeat(1, heads)                   # the head mean's backward: g / H to every head
        gy = ops.hattn_hop(inc.by_dst, a_e, g, heads, inc.n_dst, r=D)
        gz, gav, ge_e = ops.hattn_bwd_vertex(inc.by_src, inc.pos_dst_of_src(), a_v, av, ae, m, l, slope, z, g, y_e, gy, D, B)
        gae = ops.hattn_bwd_edge(inc.by_dst, ge_e, inc.n_dst)
        return gz, gav, gae, gb, None, None, None, None, None, None, None, None, None


def hattn_propagate(z: Tensor, av: Tensor, ae: Tensor, inc: Incidence, heads: int, D: Tensor, B: Tensor, negative_slope: float = 0.2,
                    concat: bool = True, bias: Optional[Tensor] = None, act: Optional[str] = None, p_attn: float = 0.0,
                    p: float = 0.0) -> Tensor:
    """The two hops of the hypergraph attention conv (reference layers.py:426-476) over ``inc`` (sources = vertices, targets =
    hyperedges).  With ``l_j = leaky_relu(av[v_j, h] + ae[e_j, h])``, ``alpha_j`` its softmax over the incidences OF VERTEX ``v_j``
    (torch_geometric's, 1e-16 in the denominator) and ``a_j = alpha_j * keep_j / (1 - p_attn)``:
    ``Y[e, h] = B[e] * sum_{j in e} a_j z[v_j, h]``, ``U[v, h] = D[v] * sum_{j ni v} a_j Y[e_j, h]``, and the result is
    ``drop_p(act(U + bias))`` with the heads side by side (``concat``) or averaged.  ``z`` [n_v, heads * C]; ``av`` [n_v, heads] and
    ``ae`` [n_e, heads] the per-row logit terms (``<z[v, h], att_v[h]>`` and ``<ze[e, h], att_e[h]>``: the edge-side table enters only
    through ``ae``); ``D`` [n_v], ``B`` [n_e] constants.  ``keep`` is the library's hash mask on (position of the incidence in the edge
    list ``inc`` was built from) * heads + head -- ``dense.dropout_scale((nnz, heads), p_attn, seed, device)`` rebuilds it; ``act``
    None / 'relu' / 'elu'; ``p`` the dropout probability on the OUTPUT.  Differentiable in ``z``, ``av``, ``ae`` and ``bias``."""
    if act not in ops.HCONV_ACTS:
        raise ValueError(f"hattn_propagate: act must be None, 'relu' or 'elu', got {act!r}")
    _lib.require_device(z, av, ae, D, B)
    if av.dtype != torch.float32 or ae.dtype != torch.float32:
        av, ae = av.float(), ae.float()
    return _HattnPropagate.apply(z, av, ae, bias, inc, int(heads), D, B, float(negative_slope), bool(concat), act, float(p_attn),
                                 float(p))


# ---- UniGCNII: the E->V hop with GCNII's initial-residual step (csrc/unigcn.hip) ---------------------------------------------------
class _GradSink:
    """Where the hops of one forward add their ``alpha * gXi`` in place: ``x0`` feeds every layer, its gradient is one buffer."""

    def __init__(self):
        self.acc: Optional[Tensor] = None

    def add(self, g: Tensor, alpha: float) -> None:
        if self.acc is None:
            self.acc = g * alpha
        else:
            self.acc.add_(g, alpha=alpha)


class _InitialResidual(torch.autograd.Function):
    """Identity on ``x0`` whose output carries a :class:`_GradSink`.  Every ``unigcn_hop`` that reads the output is a dependency of
    this node, so its backward runs after theirs and hands the accumulated buffer (plus whatever autograd itself summed from other
    uses of the output) to ``x0``."""

    @staticmethod
    def forward(ctx, x0, sink):
        ctx.sink = sink
        ctx.set_materialize_grads(False)
        return x0.view_as(x0)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        acc, ctx.sink.acc = ctx.sink.acc, None
        if acc is None:
            return g, None
        if g is not None:
            acc.add_(g)
        return acc, None


def initial_residual(x0: Tensor) -> Tensor:
    """``x0`` for the hops of one UniGCNII forward: they accumulate its gradient in place instead of returning one tensor each."""
    if not (torch.is_grad_enabled() and x0.requires_grad):
        return x0
    sink = _GradSink()
    out = _InitialResidual.apply(x0, sink)
    out._allset_grad_sink = sink
    return out


class _UniGCNHop(torch.autograd.Function):
    """``Xi = (1 - alpha) * t * degV * (H Xe) + alpha * x0`` with ``t`` the detached row-norm scale -- one kernel forward where the
    width is built (``ops.unigcn_hop_supported``), else the ``hconv`` launch plus torch ops.  Backward: ``gXe`` is the ``hconv``
    launch over the hyperedge-major CSR with ``r = (1 - alpha) * degV * t`` (``t`` saved, a constant); ``gx0 = alpha * gXi``,
    added in place to the sink of :func:`initial_residual` when ``x0`` came from there."""

    @staticmethod
    def forward(ctx, xe, x0, inc, degV, alpha, use_norm, sink, variant):
        n_v = inc.n_src
        if xe.shape[0] != inc.n_dst:
            raise _lib.AllSetHipError(f"unigcn_hop: xe has {xe.shape[0]} rows, the incidence has {inc.n_dst} hyperedges")
        if ops.unigcn_hop_supported(xe, x0):
            xi, t = ops.unigcn_hop_fwd(inc.by_src, xe, x0, n_v, degV, alpha, use_norm, variant)
        else:                                                    # width not built: correct, unfused
            a = ops.hconv_propagate(inc.by_src, xe, n_v, s=degV)
            t = None
            if use_norm:
                nrm = a.norm(dim=1)
                t = torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
                a = a * t.unsqueeze(1)
            xi = torch.add(x0 * alpha, a, alpha=1.0 - alpha)
        ctx.save_for_backward(t)
        ctx.cfg = (inc, degV, alpha, sink)
        return xi

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (t,) = ctx.saved_tensors
        inc, degV, alpha, sink = ctx.cfg
        g = g.contiguous()
        gxe = gx0 = None
        if ctx.needs_input_grad[0]:
            r = degV * (1.0 - alpha) if t is None else degV * t * (1.0 - alpha)
            gxe = ops.hconv_propagate(inc.by_dst, g, inc.n_dst, r=r)
        if ctx.needs_input_grad[1]:
            if sink is not None:
                sink.add(g, alpha)
            else:
                gx0 = g * alpha
        return gxe, gx0, None, None, None, None, None, None


def unigcn_hop(xe: Tensor, x0: Tensor, inc: Incidence, degV: Tensor, alpha: float, use_norm: bool, variant: Optional[int] = None) -> Tensor:
    """The E->V hop of a UniGCNII layer over ``inc`` (sources = vertices, targets = hyperedges) with GCNII's initial residual:
    ``a[v] = degV[v] * sum_{e ni v} xe[e]``, ``t[v] = 1 / ||a[v]||`` (0 for a zero row; a constant of the backward, as the reference's
    ``normalize_l2``) when ``use_norm`` else 1, ``Xi[v] = (1 - alpha) * t[v] * a[v] + alpha * x0[v]``.  ``xe`` [n_dst, d], ``x0``
    [n_src, d], ``degV`` [n_src] (or [n_src, 1]).  Device fp32 only.  Differentiable in ``xe`` and ``x0``.  ``variant``: kernel
    variant override (tests)."""
    _lib.require_device(xe, x0, degV)
    if xe.dtype != torch.float32 or x0.dtype != torch.float32:
        raise _lib.AllSetHipError("unigcn_hop: fp32 tensors only")
    degV = degV.reshape(-1)
    if degV.dtype != torch.float32 or degV.numel() != inc.n_src or x0.shape[0] != inc.n_src or x0.shape[1] != xe.shape[1]:
        raise _lib.AllSetHipError(f"unigcn_hop: degV {tuple(degV.shape)} {degV.dtype} / x0 {tuple(x0.shape)} do not fit {inc.n_src} "
                                  f"vertices of width {xe.shape[1]}")
    sink = getattr(x0, "_allset_grad_sink", None)
    return _UniGCNHop.apply(xe, x0, inc, degV.contiguous(), float(alpha), bool(use_norm), sink, variant)


# ---- HyperGCN: the Laplacian approximation as a structure of roles, and its hop (csrc/hypergcn.hip) ---------------------------------
class HyperGCNStructure:
    """What one HyperGCN hop needs in place of the reference's sparse ``A = D^-1/2 (W + I) D^-1/2``: per hyperedge the extremes
    ``S`` / ``I`` of the projection (int32, -1 for an empty hyperedge), the weight ``w`` and the size; per vertex ``dinv = D^-1/2`` and
    the self coefficient ``selfc``; per incidence of ``inc.by_src`` the row ``colx`` of the per-hyperedge buffer that the E->V pass
    gathers.  ``inc``: sources = vertices, targets = hyperedges.  Every tensor is a constant of autograd."""

    def __init__(self, inc: Incidence, mediators: bool, S: Tensor, I: Tensor, w: Tensor, size: Tensor, dinv: Tensor, selfc: Tensor,
                 colx: Tensor):
        self.inc, self.mediators = inc, bool(mediators)
        self.S, self.I, self.w, self.size, self.dinv, self.selfc, self.colx = S, I, w, size, dinv, selfc, colx

    @property
    def n_pq(self) -> int:
        return (2 if self.mediators else 1) * self.inc.n_dst


def hypergcn_structure(z: Tensor, rv: Tensor, inc: Incidence, mediators: bool) -> HyperGCNStructure:
    """The structure of reference ``utils.Laplacian(V, E, z, mediators)`` for the projection vector ``rv`` [z.shape[1]]: three launches
    (projection, per-hyperedge first arg-max / arg-min in the caller's edge-list order, degrees), no host synchronisation.  ``inc``:
    the vertex -> hyperedge incidence (every (vertex, hyperedge) pair once; no singleton hyperedge under ``mediators`` --
    ``baselines.HyperGCN`` checks both at construction)."""
    _lib.require_device(z, rv)
    if z.shape[0] != inc.n_src:
        raise _lib.AllSetHipError(f"hypergcn_structure: z has {z.shape[0]} rows, the incidence has {inc.n_src} vertices")
    with torch.no_grad():
        p = ops.hypergcn_project(z.detach(), rv.detach())
        S, I, w, size = ops.hypergcn_select(inc.by_dst, p, mediators)
        dinv, selfc, colx = ops.hypergcn_degree(inc.by_src, S, I, w, size, mediators)
    return HyperGCNStructure(inc, mediators, S, I, w, size, dinv, selfc, colx)


def _identity_csr(inc: Incidence, n: int) -> ops.CSR:
    """rows = columns = 0..n-1: ``hconv_propagate`` over it is the bare epilogue (bias, activation, hash dropout)."""
    hit = getattr(inc, "_identity_csr", None)
    if hit is None or hit.n_rows != n:
        ar = torch.arange(n + 1, dtype=torch.int32, device=inc.device)
        hit = ops.CSR(ar, ar[:n].contiguous(), ar[:n].contiguous(), n, n, 1)
        inc._identity_csr = hit
    return hit


def _hypergcn_apply(x: Tensor, st: HyperGCNStructure, fused: bool, bias=None, act=None, p=0.0, seed=0, base=None, variant=None) -> Tensor:
    """``drop_p(act(A x + bias))``: the two launches of csrc/hypergcn.hip, or (``fused`` False: a width that is not built) the same
    sums composed from the ``hconv`` launches and torch ops."""
    inc = st.inc
    if fused:
        pq = ops.hypergcn_v2e(inc.by_dst, st.S, st.I, st.w, st.dinv, x, st.mediators)
        return ops.hypergcn_e2v(inc.by_src, st.colx, pq, st.dinv, st.selfc, x, bias, act, p, seed, base, variant)
    y = x * st.dinv.unsqueeze(1)
    Sl, Il = st.S.long().clamp(min=0), st.I.long().clamp(min=0)
    w = torch.where(st.S >= 0, st.w, torch.zeros_like(st.w))
    if st.mediators:
        same = (st.S == st.I)
        f = (w * torch.where(same, 2.0, 1.0)).unsqueeze(1)
        T = ops.hconv_propagate(inc.by_dst, x, inc.n_dst, r=st.dinv)
        ext = y[Sl] + torch.where(same.unsqueeze(1), torch.zeros_like(y[Il]), y[Il])
        pq = torch.stack([f * ext, f * T], dim=1).reshape(2 * inc.n_dst, x.shape[1])
    else:
        pq = w.unsqueeze(1) * (y[Sl] + y[Il])
    csr = inc.by_src._replace(col=st.colx.clamp(min=0), n_cols=pq.shape[0])
    agg = ops.hconv_propagate_w(csr, pq, inc.n_src, w=(st.colx >= 0).to(torch.float32))
    out = st.dinv.unsqueeze(1) * (agg + st.selfc.unsqueeze(1) * y)
    if bias is None and act is None and p == 0.0:
        return out
    return ops.hconv_propagate(_identity_csr(inc, inc.n_src), out, inc.n_src, bias=bias, act=act, p=p, seed=seed, seed_base=base)


class _HyperGCNPropagate(torch.autograd.Function):
    """``y = drop_p(act(A x + bias))`` with ``A`` given by a :class:`HyperGCNStructure`.  Backward: the epilogue's kernel
    (``hconv_bwd_epi``: the mask and ``act'`` from the saved output) and, ``A`` being symmetric, the same hop on the masked gradient."""

    @staticmethod
    def forward(ctx, x, bias, st, act, p, variant, fused):
        from . import dense
        seed, base = dense._seed_for(p)
        y = _hypergcn_apply(x, st, fused, bias, act, p, seed, base, variant)
        epi = act is not None or p > 0.0 or bias is not None
        ctx.save_for_backward(y if epi else None)
        ctx.cfg = (st, act, p, seed, base, epi, variant, fused)
        ctx.bias_param = bias
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        st, act, p, seed, base, epi, variant, fused = ctx.cfg
        need_b = ctx.bias_param is not None and ctx.needs_input_grad[1]
        g, gb = _epilogue_backward(gy, y, act, p, seed, base, epi, ctx.bias_param, need_b)
        gx = _hypergcn_apply(g.contiguous(), st, fused, variant=variant) if ctx.needs_input_grad[0] else None
        return gx, gb, None, None, None, None, None


def hypergcn_propagate(x: Tensor, structure: HyperGCNStructure, bias: Optional[Tensor] = None, act: Optional[str] = None,
                       p: float = 0.0, variant: Optional[int] = None, fused: Optional[bool] = None) -> Tensor:
    """One HyperGCN hop ``drop_p(act(A x + bias))`` with ``A = D^-1/2 (W + I) D^-1/2`` of ``structure`` (never materialised): a V->E
    pass writing two rows per hyperedge and the fused E->V pass.  ``x`` [n_vertices, d] device fp32; ``act`` None / 'relu'; ``p`` the
    dropout probability (the library's hash mask).  Differentiable in ``x`` and ``bias``.  ``variant``: kernel variant of the E->V
    pass (tests); ``fused``: None = the HIP hop where the width is built (``ops.hypergcn_hop_supported``) and the composition from
    ``hconv`` launches and torch ops otherwise; True insists on the HIP hop (an unbuilt width raises); False forces the composition."""
    if act not in ops.RELU_ACTS:
        raise ValueError(f"hypergcn_propagate: act must be None or 'relu', got {act!r}")
    _lib.require_device(x)
    if x.dtype != torch.float32:
        raise _lib.AllSetHipError("hypergcn_propagate: fp32 tensors only")
    if x.shape[0] != structure.inc.n_src:
        raise _lib.AllSetHipError(f"hypergcn_propagate: x has {x.shape[0]} rows, the structure has {structure.inc.n_src} vertices")
    x = ops._rowmajor(x)
    if fused is None:
        fused = ops.hypergcn_hop_supported(x)
    return _HyperGCNPropagate.apply(x, bias, structure, act, float(p), variant, bool(fused))


# ---- UniGNN: the E->V hop with the row tail, UniGAT's V->E hop with the attention logit (csrc/unignn.hip) ------------------------------
class _UniGNNHop(torch.autograd.Function):
    """``y = drop_p(act(t * (s * (H xe) + c * xs)))`` with ``t`` the detached row-norm scale -- one kernel forward where the width is
    built (``ops.unignn_hop_supported``), else the ``hconv`` launches plus torch ops (same hash mask).  Backward: the epilogue's kernel
    (only when there is an activation or dropout), ``gxe`` the ``hconv`` launch over the hyperedge-major CSR with ``r = s * t`` (``t``
    saved, a constant), ``gxs = c * t * g`` and, for a tensor ``c``, ``gc = sum_v t[v] <g[v], xs[v]>`` (torch ops)."""

    @staticmethod
    def forward(ctx, xe, xs, c_t, inc, s, c_f, use_norm, act, p, variant):
        from . import dense
        n_v = inc.n_src
        if xe.shape[0] != inc.n_dst:
            raise _lib.AllSetHipError(f"unignn_hop: xe has {xe.shape[0]} rows, the incidence has {inc.n_dst} hyperedges")
        seed, base = dense._seed_for(p)
        c = c_t.detach() if c_t is not None else c_f
        if ops.unignn_hop_supported(xe, xs):
            y, t = ops.unignn_hop_fwd(inc.by_src, xe, n_v, s, xs, c, use_norm, act, p, seed, base, variant)
        else:                                                    # width not built: correct, unfused
            a = ops.hconv_propagate(inc.by_src, xe, n_v, s=s)
            if xs is not None:
                a = a + xs * c
            t = None
            if use_norm:
                nrm = a.norm(dim=1)
                t = torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
                a = a * t.unsqueeze(1)
            y = a if (act is None and p == 0.0) else \
                ops.hconv_propagate(_identity_csr(inc, n_v), a, n_v, act=act, p=p, seed=seed, seed_base=base)
        epi = act is not None or p > 0.0
        need_c = c_t is not None and ctx.needs_input_grad[2]
        ctx.save_for_backward(t, y if epi else None, xs if need_c else None, c_t)
        ctx.cfg = (inc, s, c_f, act, p, seed, base, epi)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        t, y, xs, c_t = ctx.saved_tensors
        inc, s, c_f, act, p, seed, base, epi = ctx.cfg
        g = _epilogue_backward(gy, y, act, p, seed, base, epi)[0].contiguous()
        gxe = gxs = gc = None
        if ctx.needs_input_grad[0]:
            r = s if t is None else (t if s is None else s * t)
            gxe = ops.hconv_propagate(inc.by_dst, g, inc.n_dst, r=r)
        c = c_t if c_t is not None else c_f
        if ctx.needs_input_grad[1]:
            gxs = g * c if t is None else g * (t * c).unsqueeze(1)
        if c_t is not None and ctx.needs_input_grad[2]:
            dots = (g * xs).sum(dim=1)
            gc = (dots if t is None else dots * t).sum().reshape(c_t.shape)
        return gxe, gxs, gc, None, None, None, None, None, None, None


def unignn_hop(xe: Tensor, inc: Incidence, *, s: Optional[Tensor] = None, xs: Optional[Tensor] = None, c=1.0, use_norm: bool = False,
               act: Optional[str] = None, p: float = 0.0, variant: Optional[int] = None) -> Tensor:
    """The E->V hop of a UniGNN conv over ``inc`` (sources = vertices, targets = hyperedges) with the row tail in the same launch:
    ``a[v] = s[v] * sum_{e ni v} xe[e] + c * xs[v]``, ``t[v] = 1 / ||a[v]||`` (0 for a zero row; a constant of the backward, as the
    reference's ``normalize_l2``) when ``use_norm`` else 1, ``y[v] = drop_p(act(t[v] * a[v]))``.  ``xe`` [n_dst, d]; ``s`` [n_src] (or
    [n_src, 1]) and ``xs`` [n_src, d] optional; ``c`` a float or a one-element device tensor (read on the device: a captured graph sees
    its current value); ``act`` None / 'relu'; ``p`` the dropout probability (the library's hash mask).  Device fp32 only.
    Differentiable in ``xe``, ``xs`` and a tensor ``c``.  ``variant``: kernel variant override (tests)."""
    if act not in ops.RELU_ACTS:
        raise ValueError(f"unignn_hop: act must be None or 'relu', got {act!r}")
    c_t = c if torch.is_tensor(c) else None
    _lib.require_device(xe, xs, s, c_t)
    if xe.dtype != torch.float32 or (xs is not None and xs.dtype != torch.float32) or (c_t is not None and c_t.dtype != torch.float32):
        raise _lib.AllSetHipError("unignn_hop: fp32 tensors only")
    if s is not None:
        s = s.reshape(-1)
        if s.dtype != torch.float32 or s.numel() != inc.n_src:
            raise _lib.AllSetHipError(f"unignn_hop: s {tuple(s.shape)} {s.dtype} does not fit {inc.n_src} vertices")
        s = s.contiguous()
    if xs is not None and (xs.shape[0] != inc.n_src or xs.shape[1] != xe.shape[1]):
        raise _lib.AllSetHipError(f"unignn_hop: xs {tuple(xs.shape)} does not fit {inc.n_src} vertices of width {xe.shape[1]}")
    if c_t is not None and c_t.numel() != 1:
        raise _lib.AllSetHipError(f"unignn_hop: c has {c_t.numel()} elements, expected one")
    return _UniGNNHop.apply(xe, xs, c_t, inc, s, 1.0 if c_t is not None else float(c), bool(use_norm), act, float(p), variant)


class _UniGATEdge(torch.autograd.Function):
    """``xe = s * (H^T x)``, ``ae[e, h] = <xe[e, h, :], att_e[h, :]>`` -- one kernel forward where the shape is built
    (``ops.unignn_v2e_att_supported``), else the ``hconv`` launch plus a torch reduction.  Backward (torch ops around one ``hconv``
    launch): ``gxe_total = gxe + gae (x) att_e``, ``gx`` its propagate over the vertex-major CSR with ``r = s``,
    ``gatt_e = sum_e gae[e, h] * xe[e, h, :]``."""

    @staticmethod
    def forward(ctx, x, att_e, inc, s, heads, variant):
        if x.shape[0] != inc.n_src:
            raise _lib.AllSetHipError(f"unigat_edge: x has {x.shape[0]} rows, the incidence has {inc.n_src} vertices")
        if ops.unignn_v2e_att_supported(x, heads):
            xe, ae = ops.unignn_v2e_att_fwd(inc.by_dst, x, inc.n_dst, s, att_e, heads, variant)
        else:                                                    # channels not a multiple of 4 (the class count): unfused
            xe = ops.hconv_propagate(inc.by_dst, x, inc.n_dst, s=s)
            ae = (xe.view(xe.shape[0], heads, -1) * att_e.reshape(1, heads, -1)).sum(dim=-1)
        ctx.save_for_backward(xe, att_e)
        ctx.cfg = (inc, s, heads)
        ctx.set_materialize_grads(False)
        return xe, ae

    @staticmethod
    @once_differentiable
    def backward(ctx, gxe, gae):
        xe, att_e = ctx.saved_tensors
        inc, s, heads = ctx.cfg
        gx = gatt = None
        M, d = xe.shape
        if gae is not None:
            extra = (gae.unsqueeze(-1) * att_e.reshape(1, heads, -1)).reshape(M, d)
            gxe = extra if gxe is None else gxe + extra
            if ctx.needs_input_grad[1]:
                gatt = (gae.unsqueeze(-1) * xe.view(M, heads, -1)).sum(dim=0).reshape(att_e.shape)
        if ctx.needs_input_grad[0] and gxe is not None:
            gx = ops.hconv_propagate(inc.by_src, gxe.contiguous(), inc.n_src, r=s)
        return gx, gatt, None, None, None, None


def unigat_edge(x: Tensor, inc: Incidence, s: Optional[Tensor], att_e: Tensor, heads: int, variant: Optional[int] = None
                ) -> Tuple[Tensor, Tensor]:
    """UniGAT's V->E hop over ``inc`` (sources = vertices, targets = hyperedges) with the attention logit in the same launch:
    ``xe[e] = s[e] * sum_{v in e} x[v]`` and ``ae[e, h] = <xe[e, h, :], att_e[h, :]>``.  ``x`` [n_src, heads * C]; ``s`` [n_dst] or None
    (``1 / |e|`` for the mean); ``att_e`` of ``heads * C`` elements (any shape).  Returns ``(xe [n_dst, heads * C], ae [n_dst, heads])``.
    Device fp32 only.  Differentiable in ``x`` and ``att_e``."""
    _lib.require_device(x, s, att_e)
    if x.dtype != torch.float32 or att_e.dtype != torch.float32:
        raise _lib.AllSetHipError("unigat_edge: fp32 tensors only")
    heads = int(heads)
    if heads <= 0 or x.shape[1] % heads != 0 or att_e.numel() != x.shape[1]:
        raise _lib.AllSetHipError(f"unigat_edge: x of width {x.shape[1]} / att_e of {att_e.numel()} elements do not fit {heads} heads")
    if s is not None:
        s = s.reshape(-1)
        if s.dtype != torch.float32 or s.numel() != inc.n_dst:
            raise _lib.AllSetHipError(f"unigat_edge: s {tuple(s.shape)} {s.dtype} does not fit {inc.n_dst} hyperedges")
        s = s.contiguous()
    return _UniGATEdge.apply(ops._rowmajor(x), att_e, inc, s, heads, variant)


def unignn_row_tail(a: Tensor, skip: Optional[Tensor] = None, use_norm: bool = False, act: Optional[str] = None, p: float = 0.0) -> Tensor:
    """UniGAT's row tail behind the attention pooling: ``t = 1 / ||a||`` (detached, 0 for a zero row) under ``use_norm``,
    ``y = drop_p(act(t * a + skip))`` -- the reference normalises first and adds the skip term afterwards.  Without norm and skip this
    is the one-pass ``dense.relu_dropout``; otherwise the norm and the sum are torch ops over [N, d] and only the ``relu`` + dropout
    pass is the library's (no fused kernel for this tail yet: DESIGN.md section 14 lists the passes it leaves)."""
    from . import dense
    if act not in ops.RELU_ACTS:
        raise ValueError(f"unignn_row_tail: act must be None or 'relu', got {act!r}")
    _lib.require_device(a, skip)
    if a.dtype != torch.float32 or (skip is not None and skip.dtype != torch.float32):
        raise _lib.AllSetHipError("unignn_row_tail: fp32 tensors only")
    if use_norm:
        nrm = a.detach().norm(dim=1, keepdim=True)
        a = a * torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
    if skip is not None:
        a = a + skip
    if act == 'relu':
        return dense.relu_dropout(a, p)
    return dense.hash_dropout(a, p, p > 0.0)


# ---- HAN baseline: the DGL-style attention hop and the semantic attention (csrc/han.hip) ---------------------------------------------
class _HanPropagate(torch.autograd.Function):
    """``y = elu(sum_j softmax_j(lrelu(el[s_j] + er[t])) * keep_j / (1 - p) * x[s_j] + bias)`` -- one kernel forward, written into
    column block ``block`` of ``out`` when one is given (``out`` is then returned, marked dirty).  Backward: one pass over the target
    rows (elu', the softmax statistics, the whole of ``ger``), one gather pass over the source-major CSR (``gx``, ``gel``) that
    regenerates the edge mask from the seed.  Saved: ``x``, ``el``, ``er``, the positive-logit part of the aggregate (``outpos``
    [n, H*C], ``ppos`` [n, H]) and ``lse``; ``y`` is read back where it was written.  ``graph`` is a ``han.MetapathGraph`` or a
    ``han_sampling.Block`` (both carry the two CSR orientations): ``x`` / ``el`` / ``gx`` / ``gel`` have one row per source node,
    ``er`` and everything else one per target node (``n``); the callers below have checked both counts against ``graph``."""

    @staticmethod
    def forward(ctx, x, el, er, bias, graph, heads, slope, p, out, block):
        from . import dense
        n, d = er.shape[0], x.shape[1]
        seed, base = dense._seed_for(p)
        want = any(ctx.needs_input_grad[:4])
        if out is None:
            ret = torch.empty((n, d), dtype=torch.float32, device=x.device)
            y = ret
        else:
            if out.dim() != 2 or out.shape[0] != n or out.shape[1] < (block + 1) * d or out.stride(1) != 1 or out.dtype != torch.float32:
                raise _lib.AllSetHipError(f"HAN hop: out {tuple(out.shape)} cannot hold block {block} of width {d} for {n} rows")
            ctx.mark_dirty(out)
            ret = out
            y = out.detach()[:, block * d:(block + 1) * d]
        outpos, ppos, lse = ops.han_hop_fwd(graph.rowptr, graph.col, x, el, er, heads, slope, bias, p, seed, base, y, want)
        # the output itself when it is this call's own tensor (saved the regular way: version-checked, no reference cycle); of a
        # stacked buffer only a detached alias of the block can be kept -- later hops write OTHER columns of the same storage, so
        # its version counter moves legitimately and cannot be checked: the caller must leave a written block alone until backward
        ctx.save_for_backward(x, el, er, bias, outpos, ppos, lse, ret if out is None else None)
        ctx.y_block = y if out is not None else None
        ctx.cfg = (graph, heads, slope, p, seed, base, block, d, out is not None)
        return ret

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        x, el, er, bias, outpos, ppos, lse, y_own = ctx.saved_tensors
        graph, heads, slope, p, seed, base, block, d, stacked = ctx.cfg
        if gout.stride(1) != 1:
            gout = gout.contiguous()
        gy = gout[:, block * d:(block + 1) * d] if stacked else gout
        g, stats, ger = ops.han_hop_bwd_stats(ctx.y_block if stacked else y_own, bias, gy, outpos, ppos, lse, slope)
        gx, gel = ops.han_hop_bwd_src(graph.rowptrT, graph.colT, graph.slotT, x, el, er, g, stats, slope, p, seed, base)
        gb = g.sum(0) if (bias is not None and ctx.needs_input_grad[3]) else None
        # (towards the earlier hops of the same buffer: each reads only its own block, so the gradient goes on as it is -- the
        #  wrapper admits no other producer of an ``out`` that requires grad)
        return gx, gel, ger, gb, None, None, None, None, (gout if (stacked and ctx.needs_input_grad[8]) else None), None


def han_gat_propagate(x: Tensor, el: Tensor, er: Tensor, graph, heads: int, negative_slope: float = 0.2, bias: Optional[Tensor] = None,
                      attn_drop: float = 0.0, out: Optional[Tensor] = None, block: int = 0) -> Tensor:
    """One HAN attention hop (DGL 0.7.1 ``GATConv``'s message passing + bias + ELU) over ``graph`` (a ``han.MetapathGraph``: ``n``
    nodes, edges source -> target, duplicates allowed, every node with an incoming edge): with ``e_j = leaky_relu(el[s_j, h] +
    er[t, h])``, ``p_j`` its softmax over the edges into ``t`` (no epsilon) and ``a_j = p_j * keep_j / (1 - attn_drop)``,
    ``y[t, h] = elu(sum_j a_j x[s_j, h] + bias[h])``.  ``x`` [n, heads * C], ``el`` / ``er`` [n, heads]; ``keep_j`` is the library's
    hash mask on (the edge's slot in the target-major CSR, head) -- :func:`han_edge_keep` returns it.  With ``out`` ([n, >= (block +
    1) * heads * C], row-major) the result is written into its column block ``block`` and ``out`` itself is returned: the stacked
    [n, M, heads * C] tensor of the HAN layer is filled hop by hop without a ``torch.stack`` copy.  ``out`` is a plain buffer (no
    grad) or the result of earlier calls of this function (or of :func:`han_block_propagate`: the two share one autograd Function,
    and the row counts still have to agree) into OTHER blocks of it; every block is written once and left alone until the backward
    has run.  Differentiable in ``x``, ``el``, ``er`` and ``bias``."""
    if x.shape[0] != graph.n:
        raise _lib.AllSetHipError(f"han_gat_propagate: x has {x.shape[0]} rows, the graph has {graph.n} nodes")
    return _han_propagate("han_gat_propagate", x, el, er, graph, heads, negative_slope, bias, attn_drop, out, block)


def _han_propagate(who, x, el, er, graph, heads, negative_slope, bias, attn_drop, out, block) -> Tensor:
    _lib.require_device(x, el, er)
    if out is not None and out.requires_grad and type(out.grad_fn).__name__ != "_HanPropagateBackward":
        raise ValueError(f"{who}: out must be a buffer that does not require grad, or the result of an earlier han_gat_propagate / "
                         "han_block_propagate into another of its blocks (the overwritten block would need a zero gradient)")
    if el.dtype != torch.float32 or er.dtype != torch.float32:
        el, er = el.float(), er.float()
    return _HanPropagate.apply(x, el, er, bias, graph, int(heads), float(negative_slope), float(attn_drop), out, int(block))


def han_edge_keep(graph, heads: int, p: float, seed: int) -> Tensor:
    """The hop's per-(edge, head) factor ``keep / (1 - p)`` for host seed ``seed``, [nnz, heads] in the order of the caller's edge
    list (``graph.src`` / ``graph.dst``)."""
    from . import dense
    k = dense.dropout_scale((graph.nnz, int(heads)), p, seed, graph.rowptr.device)      # indexed by target-major slot
    out = torch.empty_like(k)
    out[graph.perm.long()] = k
    return out


class _SemanticAttention(torch.autograd.Function):
    """``out[n] = sum_m softmax_m(mean_n q . tanh(W1 z[n, m] + b1)) z[n, m]``: the 128-wide hidden lives in registers, forward and
    backward (recomputed there).  Saved: ``z``, the parameters and ``{w, beta}``."""

    @staticmethod
    def forward(ctx, z, W1, b1, q):
        out, wbeta = ops.han_sem_fwd(z, W1, b1, q)
        ctx.save_for_backward(z, W1, b1, q, wbeta)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, gout):
        z, W1, b1, q, wbeta = ctx.saved_tensors
        gz, gW1, gb1, gq = ops.han_sem_bwd(z, W1, b1, q, wbeta, gout)
        return gz, gW1, gb1, gq.view_as(q)


def semantic_attention(z: Tensor, W1: Tensor, b1: Tensor, q: Tensor) -> Tensor:
    """HAN's semantic attention (reference DGL_HAN/model.py ``SemanticAttention.forward``) over stacked metapath embeddings ``z``
    [N, M, D] (contiguous): ``s[n, m] = q . tanh(W1 z[n, m] + b1)``, ``beta = softmax_m(mean_n s[n, m])``, result ``sum_m beta_m
    z[n, m]`` [N, D].  ``W1`` [128, D], ``b1`` [128], ``q`` [128] (or [1, 128]).  Built for hidden 128, D <= 128, M <= 32.
    Differentiable in all four."""
    _lib.require_device(z, W1, b1, q)
    return _SemanticAttention.apply(z, W1, b1, q)


# ---- mini-batch HAN: the attention hop over a bipartite block (csrc/han_sample.hip) ---------------------------------------------------
def han_block_propagate(x: Tensor, el: Tensor, er: Tensor, blk, heads: int, negative_slope: float = 0.2, bias: Optional[Tensor] = None,
                        attn_drop: float = 0.0, out: Optional[Tensor] = None, block: int = 0) -> Tensor:
    """:func:`han_gat_propagate` over a bipartite block ``blk`` (a ``han_sampling.Block``: ``n_src`` source nodes of which the first
    ``n_dst`` are the targets, edges source -> target in both CSR orientations): ``x`` [n_src, heads * C], ``el`` [n_src, heads],
    ``er`` [n_dst, heads]; the result has ``n_dst`` rows, ``y[t, h] = elu(sum_j a_j x[s_j, h] + bias[h])`` with ``a_j`` the softmax
    over the edges into ``t`` times the hash mask on (target-major slot, head).  ``out`` / ``block``: the stacked [n_dst, M * heads *
    C] buffer, as there.  Differentiable in ``x``, ``el``, ``er`` and ``bias``."""
    if x.shape[0] != blk.n_src or er.shape[0] != blk.n_dst:
        raise _lib.AllSetHipError(f"han_block_propagate: x has {x.shape[0]} rows and er {er.shape[0]}, the block has {blk.n_src} source "
                                  f"and {blk.n_dst} target nodes")
    return _han_propagate("han_block_propagate", x, el, er, blk, heads, negative_slope, bias, attn_drop, out, block)
