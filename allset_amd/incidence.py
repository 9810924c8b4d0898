"""Incidence structure of a hypergraph in HBM: both CSR orientations of the bipartite V-E incidence,
built ONCE on the device from the reference's ``[2, nnz]`` int64 ``edge_index``.

The reference re-derives everything from ``edge_index`` on every forward: it re-bases the hyperedge
ids in place and stacks a reversed copy (models.py:453-456), and each aggregate sizes its output from
``index.max()+1`` (layers.py:174,656) -- three device->host syncs per layer.  Here sizes are fixed at
construction; the only syncs are the one-time range checks below.

Layout (all int32, device resident):
  by_dst : CSR whose rows are the TARGETS of ``edge_index`` (row 1), cols the sources (row 0)
  by_src : the transpose (rows = sources).  One orientation is the forward CSR of a direction and the
           backward CSR of the opposite direction, so a V->E->V layer needs exactly these two.
  perm   : CSR position -> position in the caller's edge list (routes ``norm`` / attention weights).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import _lib, _memo, ops
from .ops import CSR

Tensor = torch.Tensor


class Incidence:
    """A directed bipartite incidence ``src -> dst`` with both CSR orientations.

    ``n_dst`` follows the reference's sizing rule unless given: ``index.max()+1``.
    ``n_src`` is the row count of the feature matrix that will be gathered from.
    """

    def __init__(self, by_dst: CSR, by_src: CSR, n_src: int, n_dst: int, src_extent: int, dst_extent: int):
        self.by_dst, self.by_src = by_dst, by_src
        self.n_src, self.n_dst = int(n_src), int(n_dst)
        # (max id)+1 on each side: the fewest rows a gathered matrix may have / the reference's n_dst
        self.src_extent, self.dst_extent = int(src_extent), int(dst_extent)
        self.nnz = by_dst.nnz
        self.device = by_dst.rowptr.device
        self._pos_dst_of_src: Optional[Tensor] = None     # by_src position -> by_dst position
        self._inv_cnt: Dict[str, Tensor] = {}
        self._routed: Optional[Tuple] = None              # weights(): (_memo.Stamp of the norm, its routed pair, probed for all ones)
        self._reversed: Optional["Incidence"] = None

    # ---- construction ---------------------------------------------------------------------
    @staticmethod
    def from_edge_index(edge_index: Tensor, n_src: Optional[int] = None, n_dst: Optional[int] = None,
                        src_base: int = 0, dst_base: int = 0) -> "Incidence":
        """``edge_index``: int64 [2, nnz] on a ROCm device; row 0 = source ids, row 1 = target ids.
        ids are taken relative to ``src_base`` / ``dst_base``."""
        _lib.require_device(edge_index)
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError(f"edge_index must be int64 [2, nnz], got {edge_index.dtype} {tuple(edge_index.shape)}")
        src, dst = edge_index[0].contiguous(), edge_index[1].contiguous()
        nnz = src.numel()
        if nnz > 0:   # one-time host syncs: id ranges (the kernels cannot report a bad id)
            lo_s, hi_s = int(src.min()) - src_base, int(src.max()) - src_base
            lo_d, hi_d = int(dst.min()) - dst_base, int(dst.max()) - dst_base
        else:
            lo_s = lo_d = 0
            hi_s = hi_d = -1
        if n_src is None:
            n_src = hi_s + 1
        if n_dst is None:
            n_dst = hi_d + 1                      # the reference's index.max()+1
        if lo_s < 0 or hi_s >= n_src:
            raise ValueError(f"source ids span [{lo_s}, {hi_s}] but n_src = {n_src}")   # PyG: index_select error
        if lo_d < 0 or hi_d >= n_dst:
            raise ValueError(f"target ids span [{lo_d}, {hi_d}] but n_dst = {n_dst}")
        by_dst = ops.csr_build(dst, src, dst_base, src_base, n_dst, n_src)
        by_src = ops.csr_build(src, dst, src_base, dst_base, n_src, n_dst)
        return Incidence(by_dst, by_src, n_src, n_dst, hi_s + 1, hi_d + 1)

    def reversed(self, n_dst: Optional[int] = None) -> "Incidence":
        """The opposite direction (dst -> src) sharing the same two CSRs.  ``n_dst`` of the reversed
        direction defaults to the reference's rule: (max source id)+1, which may be smaller than
        ``n_src`` when trailing rows are isolated (Q1: such vertices vanish from the E->V output)."""
        if n_dst is not None:
            return self._make_reversed(n_dst)
        if self._reversed is None:
            self._reversed = self._make_reversed(self.src_extent)
        return self._reversed

    def _make_reversed(self, n_dst: int) -> "Incidence":
        if n_dst > self.by_src.n_rows:
            raise ValueError("reversed(): n_dst exceeds the number of source rows")
        return Incidence(self.by_src, self.by_dst, self.n_dst, n_dst, self.dst_extent, self.src_extent)

    # ---- derived index maps (lazy, cached) -------------------------------------------------
    def pos_dst_of_src(self) -> Tensor:
        """int32[nnz]: for each position of ``by_src``, the position of the same incidence in ``by_dst``."""
        if self._pos_dst_of_src is None:
            inv = torch.empty(self.nnz, dtype=torch.int32, device=self.device)
            inv[self.by_dst.perm.long()] = torch.arange(self.nnz, dtype=torch.int32, device=self.device)
            self._pos_dst_of_src = inv[self.by_src.perm.long()].contiguous()
        return self._pos_dst_of_src

    def perm_dst_long(self) -> Tensor:
        """``by_dst.perm`` as int64 (what ``index_select`` takes), made once."""
        if getattr(self, "_perm_dst_long", None) is None:
            self._perm_dst_long = self.by_dst.perm.long()
        return self._perm_dst_long

    def perm_src_long(self) -> Tensor:
        """``by_src.perm`` as int64, made once."""
        if getattr(self, "_perm_src_long", None) is None:
            self._perm_src_long = self.by_src.perm.long()
        return self._perm_src_long

    def inv_perm_dst(self) -> Tensor:
        """int64[nnz]: position in ``by_dst`` of each incidence of the caller's edge list (the inverse of ``by_dst.perm``)."""
        if getattr(self, "_inv_perm_dst", None) is None:
            inv = torch.empty(self.nnz, dtype=torch.int64, device=self.device)
            inv[self.perm_dst_long()] = torch.arange(self.nnz, dtype=torch.int64, device=self.device)
            self._inv_perm_dst = inv
        return self._inv_perm_dst

    def inv_perm_src(self) -> Tensor:
        """int64[nnz]: position in ``by_src`` of each incidence of the caller's edge list (the inverse of ``by_src.perm``)."""
        if getattr(self, "_inv_perm_src", None) is None:
            inv = torch.empty(self.nnz, dtype=torch.int64, device=self.device)
            inv[self.perm_src_long()] = torch.arange(self.nnz, dtype=torch.int64, device=self.device)
            self._inv_perm_src = inv
        return self._inv_perm_src

    def inv_count_by_src(self) -> Tensor:
        """f32[nnz] in ``by_src`` order: 1 / max(|segment of the incidence's target|, 1) (mean backward)."""
        if "src" not in self._inv_cnt:
            rp = self.by_dst.rowptr
            cnt = (rp[1:] - rp[:-1]).clamp(min=1).to(torch.float32)
            self._inv_cnt["src"] = (1.0 / cnt)[self.by_src.col.long()].contiguous()
        return self._inv_cnt["src"]

    # ---- per-incidence weights ---------------------------------------------------------------
    def weights(self, norm: Optional[Tensor]) -> Tuple[Optional[Tensor], Optional[Tensor]]:
        """Route the reference's per-incidence ``norm`` (edge-list order; int64 ones by default,
        preprocessing.py:454) into (by_dst order, by_src order) f32 arrays.  All-ones -> (None, None):
        (integer norms on first sight, a persistent floating-point tensor from its second use on) the kernels then skip the weight stream.
        Kept for non-grad norms while a ``_memo.Stamp`` holds: a temporary recomputed per forward (``Importance * norm`` under ``no_grad``)
        usually gets the previous temporary's address with ``_version`` 0, and an address match alone served the FIRST weights for ever."""
        if norm is None:
            return None, None
        if norm.numel() != self.nnz:
            raise ValueError(f"norm has {norm.numel()} entries for {self.nnz} incidences")
        if norm.requires_grad:
            raise RuntimeError("weights(): a norm that requires grad is routed inside functional.deepsets_aggregate")
        entry = self._routed if (self._routed is not None and self._routed[0].holds(norm)) else None
        hit = entry[1] if entry is not None else None
        if hit is not None and not entry[2] and not _capturing(norm):
            # A floating-point norm seen a SECOND time as the very same live tensor is persistent (``torch.ones(nnz)`` kept by the
            # caller), not a per-forward temporary: probe it once now.  All ones -> the weight stream is skipped from here on.
            if bool((norm.reshape(-1) == 1).all()):
                hit = (None, None)
            self._routed = (entry[0], hit, True)
        if hit is None:
            flat = norm.reshape(-1)
            # The all-ones probe (a host sync) on FIRST sight is for the reference's DEFAULT norm only: int64 ones
            # (preprocessing.py:454), a persistent tensor probed once.  A floating-point norm is routed without looking at its
            # values the first time: under LearnMask the eval forward hands over a fresh ``Importance * norm`` temporary every call
            # (models.py:451-452), so a probe would synchronise on every forward and is illegal inside a hipGraph capture
            # (graphs.GraphedForward); a persistent float norm is probed on its second use (above).
            probed = not norm.dtype.is_floating_point
            if probed and bool((flat == 1).all()):
                hit = (None, None)
            else:
                hit = self._route(flat.to(torch.float32))
            self._routed = (_memo.Stamp(norm), hit, probed)
        return hit

    def _route(self, f: Tensor) -> Tuple[Tensor, Tensor]:
        return f.index_select(0, self.perm_dst_long()), f.index_select(0, self.perm_src_long())

    def known_unweighted(self, norm: Optional[Tensor]) -> bool:
        """``weights(norm)`` is known to be (None, None), for routes decided before the aggregation runs
        (functional.takes_packed_epilogue).  An integer norm (the reference's default) is settled by ``weights`` itself, which probes it
        on first sight whoever asks; for a floating-point norm this is a read of the cache alone -- no probe, no sync, and the cache's
        count of sightings stays what it was."""
        if norm is None:
            return True
        if norm.requires_grad or norm.numel() != self.nnz:
            return False
        if not norm.dtype.is_floating_point:
            return self.weights(norm)[0] is None
        entry = self._routed
        return entry is not None and entry[0].holds(norm) and entry[1][0] is None and entry[1][1] is None


class LeaveOneOutIncidence:
    """The structure of the exclude-self aggregation over the UNEXPANDED V->E edge list.

    The reference's ``expand_edge_index`` (preprocessing.py:22-144) turns hyperedge ``e`` of size k into k hyperedges ``e_i = e`` minus
    its i-th member; here they are never listed.  Held instead (int32; built once, on the device of ``edge_index`` -- plain torch, so
    a CPU tensor works too and is what the host tests use):

      e_rowptr, e_col : hyperedge-major CSR, members in edge-list order.  Position p of it IS the 0-based id ``expand_edge_index`` gives
                        the expanded hyperedge "(hyperedge of p) without the member at p".
      v_rowptr, v_col : vertex-major CSR whose ``col`` is that position.
      pos             : int64[nnz] position of each incidence of the caller's edge list.
      sizes           : int64[n_e] hyperedge sizes;  row_size f32[n_e] = max(k - 1, 1), the expanded hyperedges' size;
      vdeg            : f32[n_v] = sum_{e ni v} max(k_e - 1, 1), the expanded vertex degree.
      long_seg        : ids of the hyperedges longer than ``ops.loo_long_threshold()`` (one workgroup each in the kernel).

    ``n_v`` = rows of the vertex feature matrix; ``n_dst`` (fixed here) = (largest vertex id with an incidence) + 1 rows leave the
    E->V direction, the reference's sizing rule as in ``Incidence.reversed()``.  A repeated (vertex, hyperedge) pair is refused: the
    reference's dict overwrite makes it ill-defined, and the loaders coalesce such pairs away."""

    def __init__(self, edge_index: Tensor, n_v: Optional[int] = None, e_base: int = 0, long_threshold: Optional[int] = None):
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError(f"edge_index must be int64 [2, nnz], got {edge_index.dtype} {tuple(edge_index.shape)}")
        dev = edge_index.device
        v, e = edge_index[0].contiguous(), edge_index[1].contiguous() - int(e_base)
        nnz = int(v.numel())
        if nnz >= 2 ** 31 - 1:
            raise ValueError(f"{nnz} incidences do not fit the int32 CSR")
        if nnz > 0:                                   # one-time host syncs: id ranges (the kernels cannot report a bad id)
            lo_v, hi_v, lo_e, hi_e = int(v.min()), int(v.max()), int(e.min()), int(e.max())
        else:
            lo_v = lo_e = 0
            hi_v = hi_e = -1
        if n_v is None:
            n_v = hi_v + 1
        if lo_v < 0 or hi_v >= n_v:
            raise ValueError(f"vertex ids span [{lo_v}, {hi_v}] but n_v = {n_v}")
        if lo_e < 0:
            raise ValueError(f"hyperedge ids start at {lo_e + int(e_base)}, below e_base = {int(e_base)}")
        n_e = hi_e + 1
        if nnz > 0 and int(torch.unique(e * n_v + v).numel()) != nnz:
            raise ValueError("duplicate (vertex, hyperedge) incidences: the exclude-self expansion is ill-defined for them "
                             "(the reference's loaders coalesce the edge list)")
        self.n_v, self.n_e, self.n_dst, self.nnz, self.device = int(n_v), int(n_e), hi_v + 1, nnz, dev
        order_e = torch.argsort(e, stable=True)                       # members of a hyperedge in edge-list order
        self.sizes = torch.bincount(e, minlength=n_e)
        self.e_rowptr = _rowptr_of(self.sizes, dev)
        self.e_col = v[order_e].to(torch.int32).contiguous()
        self.pos = torch.empty(nnz, dtype=torch.int64, device=dev)
        self.pos[order_e] = torch.arange(nnz, dtype=torch.int64, device=dev)
        order_v = torch.argsort(v, stable=True)
        self.v_rowptr = _rowptr_of(torch.bincount(v, minlength=self.n_v), dev)
        self.v_col = self.pos[order_v].to(torch.int32).contiguous()
        self._v_of_vpos = v[order_v]                                   # vertex of each vertex-major position
        self.row_size = (self.sizes - 1).clamp(min=1).to(torch.float32)
        # (exact: integer sums far below 2^53)
        self.vdeg = torch.bincount(v, weights=self.row_size[e].double(), minlength=self.n_v).to(torch.float32) if nnz else \
            torch.zeros(self.n_v, dtype=torch.float32, device=dev)
        if long_threshold is None:
            long_threshold = ops.loo_long_threshold()
        self.long_seg = (self.sizes > long_threshold).nonzero().reshape(-1).to(torch.int32).contiguous()
        self.n_long = int(self.long_seg.numel())
        self.max_size = int(self.sizes.max()) if n_e > 0 else 0
        self._factors: Dict[Tuple[str, str], Tuple] = {}

    @staticmethod
    def from_edge_index(edge_index: Tensor, n_v: Optional[int] = None, e_base: int = 0) -> "LeaveOneOutIncidence":
        return LeaveOneOutIncidence(edge_index, n_v, e_base)

    def merge_incidence(self) -> Incidence:
        """The vertex-major CSR as an :class:`Incidence` position -> vertex (``n_src`` = nnz, ``n_dst`` = this structure's): what the
        second stage of the exclude-self PMA E->V direction pools over (functional.pma_aggregate_exclude_self).  Built on first use
        (device tensors only) and kept."""
        if getattr(self, "_merge_inc", None) is None:
            pairs = torch.stack([self.v_col.long(), self._v_of_vpos])
            self._merge_inc = Incidence.from_edge_index(pairs, n_src=self.nnz, n_dst=self.n_dst)
        return self._merge_inc

    def factors(self, aggr: str, normtype: str):
        """The :class:`LooFactors` of ``aggr`` (add | sum | mean) and ``normtype`` (all_one | deg_half_sym): what the reference
        expresses as ``norm`` and ``aggr`` over the expanded list, as scale vectors (None where all ones).
        ``norm_contruction('deg_half_sym')`` there is ``vdeg^-1/2[v] * row_size^-1/2[e_i]``, a product of a per-vertex and a
        per-hyperedge factor (every e_i of one hyperedge has the same size); ``mean`` divides by the expanded hyperedge size (V->E) or
        the expanded vertex degree (E->V).  So with a = vdeg^-1/2, b = row_size^-1/2 (ones under all_one):
          V->E:  out[(e, i)] = b_e / |e_i| * sum_{j != i} a_{n_j} x[n_j]                         -> s_src = a, s_seg = b [/ row_size]
          E->V:  out[v] = a_v / vdeg_v * sum_{e ni v} b_e * sum_{i != j(v, e)} y[(e, i)]         -> s_seg = b, w_v = a [/ vdeg] per incidence
        and each direction's backward is the other's forward with the same vectors (functional.deepsets_aggregate_exclude_self)."""
        key = (aggr, normtype)
        hit = self._factors.get(key)
        if hit is None:
            if aggr not in ("add", "sum", "mean"):
                raise NotImplementedError(f"exclude-self aggregation: aggr {aggr!r} is not built (add | sum | mean); max / min keep the "
                                          "expansion path (preprocessing.expand_edge_index)")
            if normtype not in ("all_one", "deg_half_sym"):
                raise NotImplementedError(f"exclude-self aggregation: normtype {normtype!r} is not built (all_one | deg_half_sym)")
            sym, mean = normtype == "deg_half_sym", aggr == "mean"
            has = self.vdeg > 0                                        # (a vertex without incidence is never gathered; keep it finite)
            a = torch.where(has, self.vdeg.pow(-0.5), torch.zeros_like(self.vdeg)) if sym else None
            b = self.row_size.pow(-0.5) if sym else None
            inv_deg = torch.where(has, 1.0 / self.vdeg.clamp(min=1), torch.zeros_like(self.vdeg))
            v2e_seg = (b / self.row_size if sym else 1.0 / self.row_size) if mean else b
            r = (a * inv_deg if sym else inv_deg) if mean else a       # per vertex, behind the vertex sum

            def per_incidence(t):                                      # a row scale behind the vertex sum as segreduce weights
                return t[self._v_of_vpos].contiguous() if t is not None else None
            hit = self._factors[key] = LooFactors(a, v2e_seg, per_incidence(a), b, r, per_incidence(r))
        return hit


class LooDirection(NamedTuple):
    """One direction of a :class:`LeaveOneOutIncidence`, as ``HalfNLHconv.forward`` takes it in place of an ``Incidence``."""
    loo: LeaveOneOutIncidence
    direction: str                   # 'v2e' | 'e2v'
    normtype: str = "all_one"
    attention: bool = False          # the PMA conv may take it (preprocessing.exclude_self(..., attention=True))


class LooFactors(NamedTuple):
    """The scale vectors of one (aggr, normtype); None = ones.  V->E forward: ``loo_rows(s_src=v2e_src, s_seg=v2e_seg)``, its backward:
    the vertex sum of ``loo_rows(s_seg=v2e_seg)`` weighted by ``v2e_src_inc``.  E->V forward: the vertex sum of ``loo_rows(s_seg=
    e2v_seg)`` weighted by ``e2v_row_inc``, its backward: ``loo_rows(s_src=e2v_row, s_seg=e2v_seg)``."""
    v2e_src: Optional[Tensor]        # f32[n_v]
    v2e_seg: Optional[Tensor]        # f32[n_e]
    v2e_src_inc: Optional[Tensor]    # f32[nnz], vertex-major order: v2e_src of the position's vertex
    e2v_seg: Optional[Tensor]        # f32[n_e]
    e2v_row: Optional[Tensor]        # f32[n_v]
    e2v_row_inc: Optional[Tensor]    # f32[nnz], vertex-major order


def _rowptr_of(counts: Tensor, dev) -> Tensor:
    rowptr = torch.zeros(counts.numel() + 1, dtype=torch.int32, device=dev)
    if counts.numel():
        rowptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
    return rowptr


def _capturing(t: Tensor) -> bool:
    return t.is_cuda and torch.cuda.is_current_stream_capturing()


def cached_incidence(edge_index: Tensor, n_src: Optional[int], n_dst: Optional[int] = None) -> Incidence:
    """Built on first sight of ``edge_index`` and kept on that tensor (the reference hands every forward the same one, models.py:450)."""
    return _memo.get(edge_index, "incidence", (n_src, n_dst), lambda: Incidence.from_edge_index(edge_index, n_src=n_src, n_dst=n_dst))
