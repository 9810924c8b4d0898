"""The hypergraph-convolution baselines of the reference behind its own module surface: ``HypergraphConv`` / ``HCHA`` (HGNN is
HCHA with ``symdegnorm``; with hypergraph attention: ``HypergraphAttentionConv``, ``functional.hattn_propagate``, csrc/hattn.hip) and
``HNHNConv`` / ``HNHN`` (reference layers.py:233-494, models.py:207-292).

Each conv is a Linear and two degree-scaled segment sums over the V-E incidence, V->E then E->V.  Both hops are one HIP kernel
each (``functional.scaled_propagate``, csrc/hconv.hip) with the per-row scales, the bias, the activation and the dropout that
follow them in the reference fused into the E->V launch (HNHN's ``relu`` in between into the V->E launch).  The scales are
computed once from the edge list (``preprocessing.generate_norm_HCHA`` / ``generate_norm_HNHN``) and live on the ``data`` object,
as the reference keeps HNHN's.  Device fp32 only: like the AllSet layers there is no CPU path for the propagate.

The clique-expansion baseline ``GCNConv`` / ``CEGCN`` (reference models.py:80-128) propagates over the weighted V2V graph of
``preprocessing.ConstructV2V`` + ``norm_contruction(TYPE='V2V')`` with the per-edge-weight form of the same kernel
(``functional.weighted_propagate``).  Its attention sibling ``GATConv`` / ``CEGAT`` (reference models.py:131-183) runs over the same
pairs, without weights and with one loop on every vertex, through the softmax-attention hop ``functional.gat_propagate``
(csrc/gat.hip).

``UniGCNIIConv`` / ``UniGCNII`` (reference models.py:911-996) run over the same V-E incidence as the AllSet layers: per layer a V->E
mean (``scaled_propagate`` with ``degE / |e|``), then the E->V sum with ``degV``, the optional row normalisation and GCNII's initial
residual in one launch (``functional.unigcn_hop``, csrc/unigcn.hip), then the identity-mapping step as one GEMM with the folded
weight ``(1 - beta) I + beta W`` and the one-pass ``relu`` + dropout.

``HyperGraphConvolution`` / ``HyperGCN`` (reference utils.py:11-199, models.py:29-77): the per-hyperedge Laplacian approximation is
built on the device as a structure of roles (``functional.hypergcn_structure``) and each layer is one GEMM and one two-pass hop with
the bias, ``relu`` and dropout in its second launch (``functional.hypergcn_propagate``, csrc/hypergcn.hip); the N x N adjacency is
never formed, and the re-approximating mode rebuilds the structure per layer and forward without leaving the device.

``UniGCNConv`` / ``UniGCNConv2`` / ``UniGINConv`` / ``UniSAGEConv`` / ``UniGATConv`` / ``UniGNN`` (reference models.py:601-907): the V->E
hop is ``scaled_propagate`` (UniGAT: ``functional.unigat_edge``, with the attention logit in the launch), the E->V hop
``functional.unignn_hop`` with the self term, the degree scale, the detached row normalisation, ``relu`` and dropout in its launch
(csrc/unignn.hip); UniGAT's E->V hop is the AllSet softmax pooling ``functional.pma_aggregate``.
"""
from __future__ import annotations

from types import SimpleNamespace
from typing import Optional

import math

import torch
import torch.nn as nn
from torch.nn import Parameter

from . import dense, ops
from ._lib import AllSetHipError
from .functional import (HyperGCNStructure, clique_propagate, gat_propagate, hattn_propagate, hypergcn_propagate, hypergcn_structure,
                         initial_residual, pma_aggregate, scaled_propagate, unigat_edge, unigcn_hop, unignn_hop, unignn_row_tail,
                         weighted_propagate)
from .incidence import Incidence, cached_incidence
from .layers import _linear, glorot, zeros
from .preprocessing import generate_norm_HCHA

Tensor = torch.Tensor


def _incidence(x: Tensor, edge_index) -> Incidence:
    if isinstance(edge_index, Incidence):
        return edge_index
    if not (x.is_cuda and x.dtype == torch.float32):
        raise AllSetHipError("the hypergraph-convolution baselines run on ROCm device fp32 tensors (no CPU path)")
    return cached_incidence(edge_index, n_src=x.shape[0])     # hyperedges: max(id) + 1 rows (reference layers.py:422-423)


def _hcha_scales(data, x: Tensor, symdegnorm: bool, hyperedge_weight: Optional[Tensor] = None):
    """``(D, B)`` of ``data`` for this normalisation; computed once and attached to ``data`` when it has none (or the other kind).
    With ``hyperedge_weight`` they are always computed (the weighted degree belongs to the call, not to ``data``)."""
    if hyperedge_weight is not None:
        generate_norm_HCHA(data, symdegnorm, hyperedge_weight)
    elif getattr(data, 'HCHA_D', None) is None or getattr(data, 'HCHA_symdegnorm', None) != bool(symdegnorm) \
            or data.HCHA_D.shape[0] != x.shape[0] or data.HCHA_D.device != x.device:
        generate_norm_HCHA(data, symdegnorm)
    return data.HCHA_D, data.HCHA_B


class HypergraphConv(nn.Module):
    """``X' = D^-1 H B^-1 H^T X Theta + bias`` (``symdegnorm``: ``D^-1/2 H B^-1 H^T D^-1/2 X Theta + bias``), reference
    layers.py:318-494 without attention.  ``weight`` is [in, out] (not nn.Linear's layout) and glorot-initialised, ``bias`` zeros.
    ``use_attention=True`` still raises ``NotImplementedError`` on THIS class, as it always has: the attention half of the reference's
    layer is :class:`HypergraphAttentionConv`, which shares this class's ``forward``."""

    def __init__(self, in_channels, out_channels, symdegnorm=False, use_attention=False, heads=1,
                 concat=True, negative_slope=0.2, dropout=0, bias=True, **kwargs):
        super().__init__()
        if use_attention:
            raise NotImplementedError("HypergraphConv(use_attention=True) is not built on this class: use HypergraphAttentionConv (the "
                                      "reference layer's parameters and state_dict, the attention hops of csrc/hattn.hip)")
        self._setup(in_channels, out_channels, symdegnorm, False, heads, concat, negative_slope, dropout, bias)

    def _setup(self, in_channels, out_channels, symdegnorm, use_attention, heads, concat, negative_slope, dropout, bias):
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.use_attention = bool(use_attention)
        self.symdegnorm = symdegnorm
        if self.use_attention:
            self.heads = heads
            self.concat = concat
            self.negative_slope = negative_slope
            self.dropout = dropout
            self.weight = Parameter(torch.empty(in_channels, heads * out_channels))
            self.att = Parameter(torch.empty(1, heads, 2 * out_channels))
        else:
            self.heads = 1
            self.concat = True
            self.weight = Parameter(torch.empty(in_channels, out_channels))
        if bias and concat:
            self.bias = Parameter(torch.empty(heads * out_channels))
        elif bias and not concat:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        if self.use_attention:
            glorot(self.att)
        zeros(self.bias)

    def _check(self, n_v: int, n_e: int, hyperedge_weight, hyperedge_attr) -> None:
        if hyperedge_weight is not None and (hyperedge_weight.dim() != 1 or hyperedge_weight.numel() != n_e):
            raise ValueError(f"HypergraphConv: hyperedge_weight has shape {tuple(hyperedge_weight.shape)}, expected ({n_e},)")
        if hyperedge_attr is None:
            if self.use_attention and n_e > n_v:
                raise ValueError(f"HypergraphConv: without hyperedge_attr the attention reads x[hyperedge id] (as the reference does), "
                                 f"which needs n_e <= n_v; got n_e = {n_e} hyperedges and n_v = {n_v} vertices -- pass hyperedge_attr")
        elif isinstance(hyperedge_attr, str):
            if hyperedge_attr != 'mean':
                raise ValueError(f"HypergraphConv: hyperedge_attr must be None, 'mean' or an [n_e, in_channels] tensor, got {hyperedge_attr!r}")
        elif hyperedge_attr.dim() != 2 or tuple(hyperedge_attr.shape) != (n_e, self.in_channels):
            raise ValueError(f"HypergraphConv: hyperedge_attr has shape {tuple(hyperedge_attr.shape)}, expected ({n_e}, {self.in_channels})")

    def forward(self, x: Tensor, hyperedge_index, hyperedge_weight: Optional[Tensor] = None, hyperedge_attr=None, *, scales=None,
                act: Optional[str] = None, p: float = 0.0) -> Tensor:
        """``scales`` = ``(D, B)`` from ``preprocessing.generate_norm_HCHA`` (derived from ``hyperedge_index`` and
        ``hyperedge_weight`` when None; the weight enters ``D`` only, so prebuilt scales already hold it); ``hyperedge_attr``: the
        edge-side rows of the attention (ignored without it); ``act`` / ``p``: the activation and dropout the model applies next,
        fused into the E->V launch."""
        inc = None
        if isinstance(hyperedge_index, Incidence) or x.is_cuda:
            inc = _incidence(x, hyperedge_index)
            n_e = inc.n_dst
        else:
            n_e = int(hyperedge_index[1].max()) + 1 if hyperedge_index.numel() > 0 else 0
        self._check(x.shape[0], n_e, hyperedge_weight, hyperedge_attr)
        if inc is None:
            inc = _incidence(x, hyperedge_index)               # (refuses: there is no CPU path)
        if scales is None:
            if isinstance(hyperedge_index, Incidence):
                raise ValueError("HypergraphConv: pass scales=(D, B) together with a prebuilt Incidence")
            scales = _hcha_scales(SimpleNamespace(x=x, edge_index=hyperedge_index), x, self.symdegnorm, hyperedge_weight)
        elif hyperedge_weight is not None:
            raise ValueError("HypergraphConv: scales=(D, B) already hold the hyperedge weights (generate_norm_HCHA(..., hyperedge_weight)); "
                             "pass one or the other")
        D, B = scales
        if not self.use_attention:
            xw = dense.linear(x, self.weight.t(), None)      # x Theta: the [in, out] weight read transposed by the GEMM, no copy
            if self.symdegnorm:
                h = scaled_propagate(xw, inc, 'v2e', r=D, s=B)
            else:
                h = scaled_propagate(xw, inc, 'v2e', s=B)
            return scaled_propagate(h, inc, 'e2v', s=D, bias=self.bias, act=act, p=p)
        H, C = self.heads, self.out_channels
        n_v = x.shape[0]
        att_v, att_e = self.att[:, :, :C], self.att[:, :, C:]
        if hyperedge_attr is None or isinstance(hyperedge_attr, str):
            z = dense.linear(x, self.weight.t(), None)
            # 'mean': B H^T (X Theta) = (B H^T X) Theta, one hop on the transformed rows
            ze = z[:n_e] if hyperedge_attr is None else scaled_propagate(z, inc, 'v2e', s=B)
        else:
            zz = dense.linear(torch.cat([x, hyperedge_attr.to(x.dtype)], dim=0), self.weight.t(), None)    # one GEMM for both tables
            z, ze = zz[:n_v], zz[n_v:]
        av = (z.view(n_v, H, C) * att_v).sum(dim=-1)
        ae = (ze.view(n_e, H, C) * att_e).sum(dim=-1)
        p_attn = float(self.dropout) if self.training else 0.0
        return hattn_propagate(z, av, ae, inc, H, D, B, self.negative_slope, self.concat, bias=self.bias, act=act, p_attn=p_attn, p=p)

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class HypergraphAttentionConv(HypergraphConv):
    """The reference's ``HypergraphConv(use_attention=True)`` (layers.py:377-384, 426-434, 472-480): the same parameters and
    ``state_dict`` (``weight`` [in, heads * out], ``att`` [1, heads, 2 * out] both glorot-initialised, ``bias`` zeros).  Every
    incidence (v, e) carries the coefficient ``softmax_{e ni v}(leaky_relu(<[z_v | ze_e], att>))`` per head, with dropout ``dropout``
    on it in training mode, and both hops are weighted by it (``functional.hattn_propagate``, csrc/hattn.hip); heads side by side
    (``concat``) or averaged.  The edge-side rows ``ze``: the reference reads ``z[hyperedge id]`` -- vertex rows indexed by hyperedge
    id -- which is what ``hyperedge_attr=None`` does (it needs no more hyperedges than vertices); ``hyperedge_attr`` = an [n_e, in]
    tensor gives ``ze = hyperedge_attr Theta`` (the signature of later torch_geometric releases), ``hyperedge_attr='mean'`` the mean
    of each hyperedge's member rows.  ``symdegnorm`` is refused: the reference multiplies ``D.unsqueeze(-1)`` [N, 1] into the
    [N, heads, out] view of ``x`` there, which is malformed."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0, bias=True, symdegnorm=False,
                 **kwargs):
        nn.Module.__init__(self)
        if symdegnorm:
            raise ValueError("HypergraphAttentionConv: symdegnorm=True with attention is not defined: the reference scales the "
                             "[N, heads, out] view of x by D.unsqueeze(-1) of shape [N, 1] there, which is malformed")
        self._setup(in_channels, out_channels, False, True, heads, concat, negative_slope, dropout, bias)

    def __repr__(self):
        return "{}({}, {}, heads={})".format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class HCHA(nn.Module):
    """Reference models.py:252-292: ``[in -> hidden] + [hidden -> hidden] x (L - 2) + [hidden -> classes]`` (two convs at L = 1),
    ``elu`` and dropout between convs (fused into each conv's E->V launch), nothing after the last.

    ``args.HCHA_use_attention`` (absent = off) switches every conv to hypergraph attention, wired as the reference wires its own
    multi-head baseline CEGAT: the hidden convs with ``heads=args.heads, concat=True`` (the next conv reads ``heads * MLP_hidden``
    columns), the last with ``heads=args.output_heads, concat=False``; ``args.HCHA_attn_drop`` (default 0) is the dropout on the
    coefficients.  The edge-side rows are each hyperedge's mean member row (``hyperedge_attr='mean'``): the driver's self-loop
    hyperedges make n_e > n_v, which the reference's ``x[hyperedge id]`` cannot index."""

    def __init__(self, args):
        super().__init__()
        self.num_layers = args.All_num_layers
        self.dropout = args.dropout
        self.symdegnorm = args.HCHA_symdegnorm
        self.use_attention = bool(getattr(args, 'HCHA_use_attention', False))
        self.convs = nn.ModuleList()
        if not self.use_attention:
            self.convs.append(HypergraphConv(args.num_features, args.MLP_hidden, self.symdegnorm))
            for _ in range(self.num_layers - 2):
                self.convs.append(HypergraphConv(args.MLP_hidden, args.MLP_hidden, self.symdegnorm))
            self.convs.append(HypergraphConv(args.MLP_hidden, args.num_classes, self.symdegnorm))
        else:
            heads, out_heads = int(getattr(args, 'heads', 1)), int(getattr(args, 'output_heads', 1))
            kw = dict(symdegnorm=self.symdegnorm, dropout=float(getattr(args, 'HCHA_attn_drop', 0.0)))
            self.convs.append(HypergraphAttentionConv(args.num_features, args.MLP_hidden, heads=heads, **kw))
            for _ in range(self.num_layers - 2):
                self.convs.append(HypergraphAttentionConv(heads * args.MLP_hidden, args.MLP_hidden, heads=heads, **kw))
            self.convs.append(HypergraphAttentionConv(heads * args.MLP_hidden, args.num_classes, heads=out_heads, concat=False, **kw))

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, data):
        x = data.x
        inc = _incidence(x, data.edge_index)
        scales = _hcha_scales(data, x, self.symdegnorm)
        p = float(self.dropout) if self.training else 0.0
        attr = 'mean' if self.use_attention else None
        for conv in self.convs[:-1]:
            x = conv(x, inc, hyperedge_attr=attr, scales=scales, act='elu', p=p)
        return self.convs[-1](x, inc, hyperedge_attr=attr, scales=scales)


class CEGraph:
    """The clique expansion a CEGCN forward propagates over: the edge list's two CSR orientations (``Incidence`` with ``n`` rows
    on both sides) and the edge weights routed into each CSR's order once.  Holds strong references to every tensor a captured
    graph reads."""

    def __init__(self, edge_index: Tensor, norm: Optional[Tensor], n: int):
        if not (edge_index.is_cuda and (norm is None or norm.is_cuda)):
            raise AllSetHipError("the clique-expansion baselines run on ROCm device tensors (no CPU path)")
        self.edge_index, self.norm, self.n = edge_index, norm, int(n)
        self.inc = Incidence.from_edge_index(edge_index, n_src=self.n, n_dst=self.n)
        if norm is None:
            self.w_dst = self.w_src = None
        else:
            if norm.numel() != edge_index.shape[1]:
                raise ValueError(f"CEGraph: {norm.numel()} edge weights for {edge_index.shape[1]} edges")
            w = norm.reshape(-1).to(torch.float32)
            self.w_dst = w.index_select(0, self.inc.perm_dst_long()).contiguous()
            self.w_src = w.index_select(0, self.inc.perm_src_long()).contiguous()

    def matches(self, edge_index: Tensor, norm: Optional[Tensor], n: int) -> bool:
        return self.edge_index is edge_index and self.norm is norm and self.n == n


class ImplicitCEGraph:
    """The clique expansion a CEGCN forward propagates over, NOT materialised: from the V->E list ``edge_index``
    (hyperedge ids anywhere, duplicates counting once) over ``n`` vertex rows it keeps, as int32 device tensors,

    ``e_rowptr`` / ``e_col``: the hyperedge-major CSR, members ascending (``e_col`` = vertex);
    ``v_rowptr`` / ``v_pos``: the vertex-major CSR whose columns are positions of the first;
    ``long_seg`` / ``n_long``: the hyperedges longer than ``ops.loo_long_threshold()`` (a workgroup each in ``ops.scan_rows``);
    ``deg`` (int64), ``dinv`` = ``deg^-1/2`` (float32 from the exact integer degree, inf -> 0), ``loop`` (bool: ``j < N``), ``N``,
    ``r_self`` = ``loop * dinv`` -- what ``gcn_norm`` over the expansion would give (``preprocessing.clique_implicit_structure``).

    O(nnz) index memory.  Holds strong references to every tensor a captured graph reads."""

    def __init__(self, edge_index: Tensor, n: int):
        if not edge_index.is_cuda:
            raise AllSetHipError("the clique-expansion baselines run on ROCm device tensors (no CPU path)")
        from .preprocessing import clique_implicit_structure
        st = clique_implicit_structure(edge_index, int(n))
        if int(st['e_rowptr'][-1]) >= 2 ** 31 - 1 or st['n'] >= 2 ** 31 - 1:
            raise ValueError(f"ImplicitCEGraph: {int(st['e_rowptr'][-1])} incidences do not fit an int32-indexed CSR")
        self.edge_index, self.norm, self.n = edge_index, None, int(n)
        self.nnz, self.n_e, self.N = int(st['member'].numel()), st['n_e'], st['N']
        i32 = lambda t: t.to(torch.int32).contiguous()
        self.e_rowptr, self.e_col = i32(st['e_rowptr']), i32(st['member'])
        self.v_rowptr, self.v_pos = i32(st['v_rowptr']), i32(st['v_pos'])
        size = st['e_rowptr'][1:] - st['e_rowptr'][:-1]
        self.long_seg = i32((size > ops.loo_long_threshold()).nonzero().reshape(-1))
        self.n_long = int(self.long_seg.numel())
        self.deg, self.loop = st['deg'], st['loop']
        dinv = st['deg'].to(torch.float32).pow(-0.5)
        dinv[torch.isinf(dinv)] = 0
        self.dinv = dinv.contiguous()
        self.r_self = (self.dinv * self.loop.to(torch.float32)).contiguous()

    def matches(self, edge_index: Tensor, norm: Optional[Tensor], n: int) -> bool:
        return self.edge_index is edge_index and norm is None and self.n == n


class GCNConv(nn.Module):
    """torch_geometric 1.6.3 ``GCNConv(in, out, normalize=False)`` as the reference's CEGCN builds it (models.py:94-108):
    ``out = propagate(x @ weight) + bias`` with messages from ``edge_index[0]`` into ``edge_index[1]`` scaled by the edge weight,
    over ``x.shape[0]`` output rows.  ``weight`` is [in, out], glorot-initialised; ``bias`` zeros.  The propagate, the bias and
    the activation / dropout the model applies next are one launch (``functional.weighted_propagate``, csrc/hconv.hip)."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True,
                 **kwargs):
        super().__init__()
        if normalize:
            raise NotImplementedError("GCNConv(normalize=True) is not built: normalise once with "
                                      "preprocessing.norm_contruction(data, TYPE='V2V') and pass normalize=False, as CEGCN does")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.weight = Parameter(torch.empty(in_channels, out_channels))
        if bias:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        zeros(self.bias)

    def forward(self, x: Tensor, edge_index, edge_weight: Optional[Tensor] = None, *, act: Optional[str] = None,
                p: float = 0.0) -> Tensor:
        """``edge_index``: the [2, E] int64 edge list (with ``edge_weight``), a prebuilt :class:`CEGraph`, or an
        :class:`ImplicitCEGraph` (the same hop from prefix sums over the hyperedges, ``functional.clique_propagate``); ``act`` / ``p``:
        the activation and dropout the model applies next, fused into the launch."""
        if isinstance(edge_index, ImplicitCEGraph):
            xw = dense.linear(x, self.weight.t(), None)
            return clique_propagate(xw, edge_index, bias=self.bias, act=act, p=p)
        graph = edge_index if isinstance(edge_index, CEGraph) else CEGraph(edge_index, edge_weight, x.shape[0])
        xw = dense.linear(x, self.weight.t(), None)          # x @ weight: the [in, out] weight read transposed by the GEMM, no copy
        return weighted_propagate(xw, graph.inc, graph.w_dst, graph.w_src, bias=self.bias, act=act, p=p)

    def __repr__(self):
        return "{}({}, {})".format(self.__class__.__name__, self.in_channels, self.out_channels)


class CEGCN(nn.Module):
    """Reference models.py:80-128: ``[in -> hid] + [hid -> hid] x (L - 2) + [hid -> out]`` GCN convs (two at L = 1) over the clique
    expansion (``data.edge_index`` / ``data.norm`` from ``ConstructV2V`` + ``norm_contruction(TYPE='V2V')``).  Between convs:
    ``relu``, the normalisation, dropout.  ``Normalization='bn'`` is ``BatchNorm1d(hid)``; every other value, the driver's default
    ``'ln'`` included, is ``Identity`` -- then ``relu`` and dropout ride in each non-final conv's launch.  With ``'bn'`` the ``relu``
    does, then the BatchNorm and the hash dropout (``dense.hash_dropout``) follow as their own steps."""

    def __init__(self, in_dim, hid_dim, out_dim, num_layers, dropout, Normalization='bn'):
        super().__init__()
        self.convs = nn.ModuleList()
        self.normalizations = nn.ModuleList()
        bn = Normalization == 'bn'
        self.convs.append(GCNConv(in_dim, hid_dim, normalize=False))
        self.normalizations.append(nn.BatchNorm1d(hid_dim) if bn else nn.Identity())
        for _ in range(num_layers - 2):
            self.convs.append(GCNConv(hid_dim, hid_dim, normalize=False))
            self.normalizations.append(nn.BatchNorm1d(hid_dim) if bn else nn.Identity())
        self.convs.append(GCNConv(hid_dim, out_dim, normalize=False))
        self.dropout = dropout
        self._graph = None                                   # a CEGraph, or an ImplicitCEGraph for ConstructV2V_implicit data

    def reset_parameters(self):
        for layer in self.convs:
            layer.reset_parameters()
        for normalization in self.normalizations:
            if not isinstance(normalization, nn.Identity):
                normalization.reset_parameters()

    def graph(self, data, x: Tensor):
        """The V2V graph of ``data``, built on first sight and kept (with the tensors it came from) for later forwards."""
        norm = getattr(data, 'norm', None)
        implicit = bool(getattr(data, 'clique_implicit', False))           # preprocessing.ConstructV2V_implicit: the V->E list itself
        if self._graph is None or isinstance(self._graph, ImplicitCEGraph) != implicit \
                or not self._graph.matches(data.edge_index, norm, x.shape[0]):
            self._graph = ImplicitCEGraph(data.edge_index, x.shape[0]) if implicit else CEGraph(data.edge_index, norm, x.shape[0])
        return self._graph

    def forward(self, data):
        x = data.x
        graph = self.graph(data, x)
        p = float(self.dropout) if self.training else 0.0
        for i, conv in enumerate(self.convs[:-1]):
            nm = self.normalizations[i]
            if isinstance(nm, nn.Identity):
                x = conv(x, graph, act='relu', p=p)
            else:
                x = dense.batch_norm(nm, conv(x, graph, act='relu'))
                x = dense.hash_dropout(x, p, self.training)        # the library's hash mask: reproducible, capturable
        return self.convs[-1](x, graph)


class CEGATGraph:
    """The graph a CEGAT forward attends over, as torch_geometric 1.6.3's ``GATConv`` derives it from ``edge_index`` on every call:
    existing self-loops dropped, one loop added for every one of the ``n`` vertices (isolated ones included), edge weights ignored.
    Both CSR orientations, built once; holds strong references to every tensor a captured graph reads."""

    def __init__(self, edge_index: Tensor, n: int):
        if not edge_index.is_cuda:
            raise AllSetHipError("the clique-expansion baselines run on ROCm device tensors (no CPU path)")
        self.edge_index, self.n = edge_index, int(n)
        keep = edge_index[0] != edge_index[1]
        loops = torch.arange(self.n, dtype=edge_index.dtype, device=edge_index.device)
        self.attention_index = torch.cat([edge_index[:, keep], loops.unsqueeze(0).repeat(2, 1)], dim=1).contiguous()
        self.inc = Incidence.from_edge_index(self.attention_index, n_src=self.n, n_dst=self.n)

    def matches(self, edge_index: Tensor, n: int) -> bool:
        return self.edge_index is edge_index and self.n == n


class GATConv(nn.Module):
    """torch_geometric 1.6.3 ``GATConv`` as the reference's CEGAT builds it (models.py:147-163): ``xw = lin_l(x)`` viewed as
    ``[n, heads, C]``, ``al = (xw * att_l).sum(-1)``, ``ar = (xw * att_r).sum(-1)``, self-loops removed and one added per vertex,
    ``e = leaky_relu(al[source] + ar[target])`` softmax-normalised over each target's incoming edges, ``out[target] = sum e * xw[source]``,
    heads concatenated (``concat``) or averaged, then ``+ bias``.  ``lin_r`` is the same module object as ``lin_l`` (one weight, two
    names in the ``state_dict``).  The hop, the bias and the activation / dropout the model applies next are one launch
    (``functional.gat_propagate``, csrc/gat.hip).  Dropout on the attention coefficients and bipartite inputs are not built."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, **kwargs):
        super().__init__()
        if not isinstance(in_channels, int):
            raise NotImplementedError("GATConv: bipartite (in_l, in_r) inputs are not built (the reference never uses them)")
        if dropout > 0.0:
            raise NotImplementedError("GATConv: dropout on the attention coefficients is not built (the reference never sets it)")
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.heads = heads
        self.concat = concat
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.add_self_loops = add_self_loops
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = Parameter(torch.empty(1, heads, out_channels))
        self.att_r = Parameter(torch.empty(1, heads, out_channels))
        if bias and concat:
            self.bias = Parameter(torch.empty(heads * out_channels))
        elif bias and not concat:
            self.bias = Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.lin_l.weight)
        glorot(self.lin_r.weight)            # the same tensor drawn a second time, as 1.6.3 does: it consumes RNG state
        glorot(self.att_l)
        glorot(self.att_r)
        zeros(self.bias)

    def forward(self, x: Tensor, edge_index, *, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        """``edge_index``: the [2, E] int64 edge list or a prebuilt :class:`CEGATGraph`; ``act`` / ``p``: the activation and dropout
        the model applies next, fused into the launch."""
        if isinstance(x, (tuple, list)):
            raise NotImplementedError("GATConv: bipartite (x_l, x_r) inputs are not built (the reference never uses them)")
        if isinstance(edge_index, CEGATGraph):
            graph = edge_index
        elif self.add_self_loops:
            graph = CEGATGraph(edge_index, x.shape[0])
        else:
            graph = SimpleNamespace(inc=Incidence.from_edge_index(edge_index, n_src=x.shape[0], n_dst=x.shape[0]))
        H, C = self.heads, self.out_channels
        xw = dense.linear(x, self.lin_l.weight, None)
        xh = xw.view(-1, H, C)
        al = (xh * self.att_l).sum(dim=-1)
        ar = (xh * self.att_r).sum(dim=-1)
        return gat_propagate(xw, al, ar, graph.inc, H, self.negative_slope, self.concat, bias=self.bias, act=act, p=p)

    def __repr__(self):
        return "{}({}, {}, heads={})".format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class CEGAT(nn.Module):
    """Reference models.py:131-183: ``GATConv(in, hid, heads)``, ``GATConv(heads * hid, hid)`` x (L - 2),
    ``GATConv(heads * hid, out, heads=output_heads, concat=False)`` (two convs at L = 1) over the clique expansion's pairs
    (``data.edge_index`` from ``ConstructV2V`` + ``norm_contruction(TYPE='V2V')``; ``data.norm`` is ignored, as in the reference).
    Between convs: ``relu``, the normalisation, dropout -- fused into the hop with ``Identity``; with ``'bn'`` the ``relu`` is, then
    ``dense.batch_norm`` and ``dense.hash_dropout`` follow, as in :class:`CEGCN`.

    The reference's module fails at its first forward for two families of arguments, refused here at construction:
    ``num_layers > 2`` with ``heads > 1`` (a middle conv emits ``hid`` columns, the next expects ``heads * hid``) and
    ``Normalization='bn'`` with ``heads > 1`` (``BatchNorm1d(hid)`` applied to ``heads * hid`` columns)."""

    def __init__(self, in_dim, hid_dim, out_dim, num_layers, heads, output_heads, dropout, Normalization='bn'):
        super().__init__()
        bn = Normalization == 'bn'
        if num_layers > 2 and heads > 1:
            raise ValueError(f"CEGAT: num_layers={num_layers} with heads={heads} cannot run (in the reference either): the middle "
                             f"convs emit hid_dim={hid_dim} columns but the conv behind them expects heads * hid_dim={heads * hid_dim}")
        if bn and heads > 1:
            raise ValueError(f"CEGAT: Normalization='bn' with heads={heads} cannot run (in the reference either): BatchNorm1d({hid_dim}) "
                             f"meets the first conv's heads * hid_dim={heads * hid_dim} columns")
        self.convs = nn.ModuleList()
        self.normalizations = nn.ModuleList()
        self.convs.append(GATConv(in_dim, hid_dim, heads))
        self.normalizations.append(nn.BatchNorm1d(hid_dim) if bn else nn.Identity())
        for _ in range(num_layers - 2):
            self.convs.append(GATConv(heads * hid_dim, hid_dim))
            self.normalizations.append(nn.BatchNorm1d(hid_dim) if bn else nn.Identity())
        self.convs.append(GATConv(heads * hid_dim, out_dim, heads=output_heads, concat=False))
        self.dropout = dropout
        self._graph: Optional[CEGATGraph] = None

    def reset_parameters(self):
        for layer in self.convs:
            layer.reset_parameters()
        for normalization in self.normalizations:
            if not isinstance(normalization, nn.Identity):
                normalization.reset_parameters()

    def graph(self, data, x: Tensor) -> CEGATGraph:
        """The attention graph of ``data``, built on first sight and kept (with the tensors it came from) for later forwards."""
        if self._graph is None or not self._graph.matches(data.edge_index, x.shape[0]):
            self._graph = CEGATGraph(data.edge_index, x.shape[0])
        return self._graph

    def forward(self, data):
        x = data.x
        graph = self.graph(data, x)
        p = float(self.dropout) if self.training else 0.0
        for i, conv in enumerate(self.convs[:-1]):
            nm = self.normalizations[i]
            if isinstance(nm, nn.Identity):
                x = conv(x, graph, act='relu', p=p)
            else:
                x = dense.batch_norm(nm, conv(x, graph, act='relu'))
                x = dense.hash_dropout(x, p, self.training)        # the library's hash mask: reproducible, capturable
        return self.convs[-1](x, graph)


class HNHNConv(nn.Module):
    """Reference layers.py:233-316: ``x = D_v_beta * weight_v2e(x)``, ``h = D_e_beta_inv * sum_{v in e} x_v`` (``relu`` if
    ``nonlinear_inbetween``), ``h = D_e_alpha * weight_e2v(h)``, ``out = D_v_alpha_inv * sum_{e ni v} h_e``.  The norms come from
    ``data`` (``preprocessing.generate_norm_HNHN``)."""

    def __init__(self, in_channels, hidden_channels, out_channels, heads=1, nonlinear_inbetween=True,
                 concat=True, bias=True, **kwargs):
        super().__init__()
        self.in_channels = in_channels
        self.hidden_channels = hidden_channels
        self.out_channels = out_channels
        self.nonlinear_inbetween = nonlinear_inbetween
        self.heads = heads
        self.concat = True
        self.weight_v2e = nn.Linear(in_channels, hidden_channels)
        self.weight_e2v = nn.Linear(hidden_channels, out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        self.weight_v2e.reset_parameters()
        self.weight_e2v.reset_parameters()

    def forward(self, x: Tensor, data, *, inc: Optional[Incidence] = None, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        for name in ('D_v_beta', 'D_e_beta_inv', 'D_e_alpha', 'D_v_alpha_inv'):
            if getattr(data, name, None) is None:
                raise ValueError(f"HNHNConv: data.{name} is missing (preprocessing.generate_norm_HNHN computes the norms)")
        inc = inc if inc is not None else _incidence(x, data.edge_index)
        h = scaled_propagate(_linear(self.weight_v2e, x), inc, 'v2e', r=data.D_v_beta, s=data.D_e_beta_inv,
                             act='relu' if self.nonlinear_inbetween else None)
        return scaled_propagate(_linear(self.weight_e2v, h), inc, 'e2v', r=data.D_e_alpha, s=data.D_v_alpha_inv, act=act, p=p)

    def __repr__(self):
        return "{}({}, {}, {})".format(self.__class__.__name__, self.in_channels, self.hidden_channels, self.out_channels)


class HNHN(nn.Module):
    """Reference models.py:207-249: one conv at L = 1 (nothing after it); otherwise ``relu`` and dropout between convs (fused
    into each conv's E->V launch)."""

    def __init__(self, args):
        super().__init__()
        self.num_layers = args.All_num_layers
        self.dropout = args.dropout
        nl = args.HNHN_nonlinear_inbetween
        self.convs = nn.ModuleList()
        if self.num_layers == 1:
            self.convs.append(HNHNConv(args.num_features, args.MLP_hidden, args.num_classes, nonlinear_inbetween=nl))
        else:
            self.convs.append(HNHNConv(args.num_features, args.MLP_hidden, args.MLP_hidden, nonlinear_inbetween=nl))
            for _ in range(self.num_layers - 2):
                self.convs.append(HNHNConv(args.MLP_hidden, args.MLP_hidden, args.MLP_hidden, nonlinear_inbetween=nl))
            self.convs.append(HNHNConv(args.MLP_hidden, args.MLP_hidden, args.num_classes, nonlinear_inbetween=nl))

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def forward(self, data):
        x = data.x
        inc = _incidence(x, data.edge_index)
        p = float(self.dropout) if self.training else 0.0
        for conv in self.convs[:-1]:
            x = conv(x, data, inc=inc, act='relu', p=p)
        return self.convs[-1](x, data, inc=inc)


class UniGraph:
    """What a UniGCNII forward propagates over: the vertex-hyperedge ``Incidence`` of the (sorted, de-duplicated) pairs ``V``, ``E``
    and the degree scales as flat device vectors -- ``degV`` [N], and ``scaleE`` [M] = ``degE / |e|`` (the V->E mean and the ``degE``
    factor as one per-row scale).  Built once; holds strong references to every tensor a captured graph reads."""

    def __init__(self, V: Tensor, E: Tensor, degV: Tensor, degE: Tensor, device):
        device = torch.device(device)
        if device.type != 'cuda':
            raise AllSetHipError("the UniGCNII baseline runs on ROCm device fp32 tensors (no CPU path)")
        self.V, self.E, self.degV_arg, self.degE_arg = V, E, degV, degE
        n, m = degV.shape[0], degE.shape[0]
        self.edge_index = torch.stack([V.reshape(-1), E.reshape(-1)]).to(device=device, dtype=torch.int64).contiguous()
        self.inc = Incidence.from_edge_index(self.edge_index, n_src=n, n_dst=m)
        self.degV = degV.to(device=device, dtype=torch.float32).reshape(-1).contiguous()
        rp = self.inc.by_dst.rowptr
        size = (rp[1:] - rp[:-1]).clamp(min=1).to(torch.float32)
        self.scaleE = (degE.to(device=device, dtype=torch.float32).reshape(-1) / size).contiguous()
        self.device = device

    def matches(self, V, E, degV, degE, device) -> bool:
        return self.V is V and self.E is E and self.degV_arg is degV and self.degE_arg is degE and self.device == torch.device(device)


def _unignn_scales(args):
    degV, degE = getattr(args, 'UniGNN_degV', None), getattr(args, 'UniGNN_degE', None)
    if not (torch.is_tensor(degV) and torch.is_tensor(degE)):
        raise ValueError("UniGCNII: args.UniGNN_degV / args.UniGNN_degE are missing (preprocessing.generate_norm_UniGNN computes them)")
    return degV, degE


class UniGCNIIConv(nn.Module):
    """Reference models.py:911-944: ``Xe = degE * mean_{v in e} X[v]``, ``Xv = degV * sum_{e ni v} Xe[e]`` (row-normalised with a
    detached norm under ``args.UniGNN_use_norm``), ``Xi = (1 - alpha) Xv + alpha X0``, ``out = (1 - beta) Xi + beta W(Xi)``.  The last
    step is ONE GEMM with the folded weight ``(1 - beta) I + beta W``, built by small torch ops that stay in autograd (``W.grad`` is
    ``beta`` times the folded weight's gradient)."""

    def __init__(self, args, in_features, out_features):
        super().__init__()
        self.W = nn.Linear(in_features, out_features, bias=False)
        self.args = args

    def reset_parameters(self):
        self.W.reset_parameters()

    def folded_weight(self, beta: float) -> Tensor:
        w = self.W.weight
        if w.shape[0] != w.shape[1]:
            raise ValueError(f"UniGCNIIConv: the identity mapping needs a square W, got {tuple(w.shape)}")
        return torch.eye(w.shape[0], dtype=w.dtype, device=w.device).mul_(1.0 - beta).add(w, alpha=beta)

    def forward(self, X: Tensor, vertex, edges, alpha, beta, X0: Tensor) -> Tensor:
        """``vertex`` / ``edges``: the pair lists, or a prebuilt :class:`UniGraph` as ``vertex`` (``edges`` is then ignored)."""
        if isinstance(vertex, UniGraph):
            graph = vertex
        else:
            degV, degE = _unignn_scales(self.args)
            graph = UniGraph(vertex, edges, degV, degE, X.device)
        Xe = scaled_propagate(X, graph.inc, 'v2e', s=graph.scaleE)
        Xi = unigcn_hop(Xe, X0, graph.inc, graph.degV, alpha, bool(getattr(self.args, 'UniGNN_use_norm', False)))
        return dense.linear(Xi, self.folded_weight(beta), None)


class UniGCNII(nn.Module):
    """Reference models.py:948-996: ``Linear(nfeat, d)`` with ``d = nhid * nhead``, ``nlayer`` :class:`UniGCNIIConv` of width ``d``,
    ``Linear(d, nclass)``; dropout 0.2 on the input, before every conv and before the last Linear, ``alpha`` = 0.1, ``lamda`` = 0.5
    (``beta_i = log(lamda / (i + 1) + 1)``), whatever ``--dropout`` says.  ``V`` / ``E``: the sorted, de-duplicated pairs of
    ``preprocessing.ConstructH_pairs``; the degree scales are read from ``args.UniGNN_degV`` / ``UniGNN_degE``.  The ``relu`` behind a
    conv and the dropout in front of the next layer are one pass (``dense.relu_dropout``); training-mode masks are the library's hash
    dropout.  ``reg_params`` (the conv weights) and ``non_reg_params`` (first and last Linear) are the reference's two optimizer groups."""

    def __init__(self, args, nfeat, nhid, nclass, nlayer, nhead, V, E):
        super().__init__()
        self.args = args
        self.V = V
        self.E = E
        nhid = nhid * nhead
        self.act = nn.ReLU()
        self.input_drop = nn.Dropout(0.6)
        self.dropout = nn.Dropout(0.2)
        self.convs = nn.ModuleList()
        self.convs.append(nn.Linear(nfeat, nhid))
        for _ in range(nlayer):
            self.convs.append(UniGCNIIConv(args, nhid, nhid))
        self.convs.append(nn.Linear(nhid, nclass))
        self.reg_params = list(self.convs[1:-1].parameters())
        self.non_reg_params = list(self.convs[0:1].parameters()) + list(self.convs[-1:].parameters())
        self._graph: Optional[UniGraph] = None

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()

    def graph(self, x: Tensor) -> UniGraph:
        """The incidence and scales on ``x``'s device, built on first sight and kept for later forwards."""
        degV, degE = _unignn_scales(self.args)
        if self._graph is None or not self._graph.matches(self.V, self.E, degV, degE, x.device):
            if degV.shape[0] != x.shape[0]:
                raise ValueError(f"UniGCNII: args.UniGNN_degV has {degV.shape[0]} rows, data.x has {x.shape[0]}")
            self._graph = UniGraph(self.V, self.E, degV, degE, x.device)
        return self._graph

    def forward(self, data):
        x = data.x
        if not (x.is_cuda and x.dtype == torch.float32):
            raise AllSetHipError("the UniGCNII baseline runs on ROCm device fp32 tensors (no CPU path)")
        graph = self.graph(x)
        lamda, alpha = 0.5, 0.1
        p = float(self.dropout.p) if self.training else 0.0
        x = dense.hash_dropout(x, p, self.training)
        x0 = initial_residual(dense.relu_dropout(_linear(self.convs[0], x), 0.0))
        x = dense.hash_dropout(x0, p, self.training)
        for i, conv in enumerate(self.convs[1:-1]):
            beta = math.log(lamda / (i + 1) + 1)
            # relu, and the dropout in front of the next layer (the next conv, or the last Linear), in one pass
            x = dense.relu_dropout(conv(x, graph, None, alpha, beta, x0), p)
        return _linear(self.convs[-1], x)


# ---- UniGNN: UniGCN, UniGCN2, UniGIN, UniSAGE, UniGAT ------------------------------------------------------------------------------
_UNIGNN_AGGREGATES = ('mean', 'sum')


class UniGNNGraph(UniGraph):
    """:class:`UniGraph` with what the five plain UniGNN convs need beside it, each as a flat device vector built once: ``degE`` alone
    (``first_aggregate='sum'``), ``inv_size`` = ``1 / |e|`` (the V->E mean of the convs without degree scales), ``inv_deg`` =
    ``1 / max(deg(v), 1)`` (UniSAGE's ``second_aggregate='mean'``), and ``inc_ev``, the hyperedge -> vertex direction of the same two
    CSRs with one output row per vertex (UniGAT's softmax pooling).  Holds strong references to every tensor a captured graph reads."""

    def __init__(self, V: Tensor, E: Tensor, degV: Tensor, degE: Tensor, device):
        super().__init__(V, E, degV, degE, device)
        self.degE = degE.to(device=self.device, dtype=torch.float32).reshape(-1).contiguous()
        re_, rv = self.inc.by_dst.rowptr, self.inc.by_src.rowptr
        self.inv_size = (1.0 / (re_[1:] - re_[:-1]).clamp(min=1).to(torch.float32)).contiguous()
        self.inv_deg = (1.0 / (rv[1:] - rv[:-1]).clamp(min=1).to(torch.float32)).contiguous()
        self.inc_ev = self.inc.reversed(n_dst=self.inc.n_src)

    def edge_scale(self, first_aggregate: str, with_degE: bool) -> Optional[Tensor]:
        """The per-hyperedge scale of the V->E hop: the mean's ``1 / |e|`` and / or ``degE``, as one vector (None = ones)."""
        if first_aggregate == 'mean':
            return self.scaleE if with_degE else self.inv_size
        return self.degE if with_degE else None


def _unignn_first_aggregate(args) -> str:
    agg = getattr(args, 'first_aggregate', 'mean')
    if agg not in _UNIGNN_AGGREGATES:
        raise NotImplementedError(f"UniGNN: first_aggregate={agg!r} is not built: the V->E hop is a sum or a mean over the members of "
                                  f"a hyperedge ({_UNIGNN_AGGREGATES})")
    return agg


def _unignn_second_aggregate(args) -> str:
    agg = getattr(args, 'second_aggregate', 'sum')
    if agg not in _UNIGNN_AGGREGATES:
        raise NotImplementedError(f"UniGNN: second_aggregate={agg!r} is not built: the E->V hop is a sum or a mean over the hyperedges "
                                  f"of a vertex ({_UNIGNN_AGGREGATES})")
    return agg


def _unignn_degrees(args):
    degV, degE = getattr(args, 'degV', None), getattr(args, 'degE', None)
    if not (torch.is_tensor(degV) and torch.is_tensor(degE)):
        raise ValueError("UniGNN: args.degV / args.degE are missing (preprocessing.generate_norm_UniGNN computes them; train.preprocess "
                         "sets both)")
    return degV, degE


def _unignn_post(x: Tensor, act: Optional[str], p: float) -> Tensor:
    """The activation and dropout behind a conv whose last step is not a hop: one pass."""
    if act == 'relu':
        return dense.relu_dropout(x, p)
    return dense.hash_dropout(x, p, p > 0.0)


class _UniConv(nn.Module):
    """What the five convs share (reference models.py:601-790): the constructor's signature and attributes, ``__repr__``, the graph
    argument.  ``forward(X, vertex, edges, *, act=None, p=0.0)``: ``vertex`` / ``edges`` are the pair lists, or ``vertex`` is a prebuilt
    :class:`UniGNNGraph` (``edges`` is then ignored); ``act`` / ``p``: the activation and dropout the model applies next, fused into the
    conv's last launch."""
    _bias = False

    def __init__(self, args, in_channels, out_channels, heads=8, dropout=0., negative_slope=0.2):
        super().__init__()
        self.W = nn.Linear(in_channels, heads * out_channels, bias=self._bias)
        self.heads = heads
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.negative_slope = negative_slope
        self.dropout = dropout
        self.args = args
        _unignn_first_aggregate(args)

    def reset_parameters(self):
        self.W.reset_parameters()

    def _graph(self, X: Tensor, vertex, edges) -> UniGNNGraph:
        if isinstance(vertex, UniGNNGraph):
            return vertex
        if not (X.is_cuda and X.dtype == torch.float32):
            raise AllSetHipError("the UniGNN baselines run on ROCm device fp32 tensors (no CPU path)")
        degV, degE = _unignn_degrees(self.args)
        return UniGNNGraph(vertex, edges, degV, degE, X.device)

    def _use_norm(self) -> bool:
        return bool(getattr(self.args, 'use_norm', False))

    def __repr__(self):
        return '{}({}, {}, heads={})'.format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class UniGCNConv(_UniConv):
    """Reference models.py:694-737: ``X = W(X)``, ``Xe = degE * agg_{v in e} X[v]``, ``Xv = degV * sum_{e ni v} Xe[e]``, row-normalised
    (detached norm) under ``args.use_norm``.  The E->V sum, ``degV``, the norm and the model's ``relu`` + dropout are one launch."""

    def forward(self, X: Tensor, vertex, edges=None, *, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        g = self._graph(X, vertex, edges)
        Xe = scaled_propagate(_linear(self.W, X), g.inc, 'v2e', s=g.edge_scale(_unignn_first_aggregate(self.args), True))
        return unignn_hop(Xe, g.inc, s=g.degV, use_norm=self._use_norm(), act=act, p=p)


class UniGCNConv2(_UniConv):
    """Reference models.py:742-788: the two hops and the norm of :class:`UniGCNConv` first, the Linear (with bias) last.  The hop
    carries the norm only; ``relu`` + dropout follow the GEMM in one pass."""
    _bias = True

    def forward(self, X: Tensor, vertex, edges=None, *, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        g = self._graph(X, vertex, edges)
        Xe = scaled_propagate(X, g.inc, 'v2e', s=g.edge_scale(_unignn_first_aggregate(self.args), True))
        Xv = unignn_hop(Xe, g.inc, s=g.degV, use_norm=self._use_norm())
        return _unignn_post(_linear(self.W, Xv), act, p)


class UniGINConv(_UniConv):
    """Reference models.py:646-689: ``X = W(X)``, ``Xe = agg_{v in e} X[v]``, ``X = (1 + eps) X + sum_{e ni v} Xe[e]``, then the norm.
    ``1 + eps`` reaches the hop as a device scalar, so a captured graph follows the parameter."""

    def __init__(self, args, in_channels, out_channels, heads=8, dropout=0., negative_slope=0.2):
        super().__init__(args, in_channels, out_channels, heads, dropout, negative_slope)
        self.eps = nn.Parameter(torch.Tensor([0.]))

    def reset_parameters(self):
        self.W.reset_parameters()
        zeros(self.eps)

    def forward(self, X: Tensor, vertex, edges=None, *, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        g = self._graph(X, vertex, edges)
        X = _linear(self.W, X)
        Xe = scaled_propagate(X, g.inc, 'v2e', s=g.edge_scale(_unignn_first_aggregate(self.args), False))
        return unignn_hop(Xe, g.inc, xs=X, c=1 + self.eps, use_norm=self._use_norm(), act=act, p=p)


class UniSAGEConv(_UniConv):
    """Reference models.py:601-641: ``X = W(X)``, ``Xe = agg_{v in e} X[v]``, ``X = X + agg2_{e ni v} Xe[e]`` with ``agg2`` =
    ``args.second_aggregate`` (sum / mean), then the norm."""

    def __init__(self, args, in_channels, out_channels, heads=8, dropout=0., negative_slope=0.2):
        super().__init__(args, in_channels, out_channels, heads, dropout, negative_slope)
        _unignn_second_aggregate(args)

    def forward(self, X: Tensor, vertex, edges=None, *, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        g = self._graph(X, vertex, edges)
        X = _linear(self.W, X)
        Xe = scaled_propagate(X, g.inc, 'v2e', s=g.edge_scale(_unignn_first_aggregate(self.args), False))
        s = g.inv_deg if _unignn_second_aggregate(self.args) == 'mean' else None
        return unignn_hop(Xe, g.inc, s=s, xs=X, c=1.0, use_norm=self._use_norm(), act=act, p=p)


class UniGATConv(_UniConv):
    """Reference models.py:792-854: ``X0 = W(X)`` as ``[N, H, C]``, ``Xe = agg_{v in e} X0[v]``, ``alpha_e = <Xe, att_e>`` per head,
    ``Xv[v] = sum_{e ni v} softmax_e(leaky_relu(alpha_e)) Xe[e]``, the norm, ``+ X0`` under ``skip_sum``.  The V->E hop writes the
    logits in its own launch (``functional.unigat_edge``); the logit depends on the gathered hyperedge alone, so the E->V hop is the
    AllSet softmax pooling (``functional.pma_aggregate``) over the hyperedge -> vertex direction.  ``att_v`` is an unused parameter, as
    in the reference.  Dropout on the attention coefficients is not built."""

    def __init__(self, args, in_channels, out_channels, heads=8, dropout=0., negative_slope=0.2, skip_sum=False):
        if dropout > 0.0:
            raise NotImplementedError("UniGATConv: dropout on the attention coefficients (attn_drop > 0) is not built")
        super().__init__(args, in_channels, out_channels, heads, dropout, negative_slope)
        self.att_v = nn.Parameter(torch.Tensor(1, heads, out_channels))
        self.att_e = nn.Parameter(torch.Tensor(1, heads, out_channels))
        self.attn_drop = nn.Dropout(dropout)
        self.leaky_relu = nn.LeakyReLU(negative_slope)
        self.skip_sum = skip_sum
        self.reset_attention()

    def reset_attention(self):
        glorot(self.att_v)
        glorot(self.att_e)

    def reset_parameters(self):
        self.W.reset_parameters()
        self.reset_attention()

    def forward(self, X: Tensor, vertex, edges=None, *, act: Optional[str] = None, p: float = 0.0) -> Tensor:
        g = self._graph(X, vertex, edges)
        H = self.heads
        X0 = _linear(self.W, X)
        Xe, ae = unigat_edge(X0, g.inc, g.edge_scale(_unignn_first_aggregate(self.args), False), self.att_e, H)
        Xv, _, _ = pma_aggregate(Xe, ae, g.inc_ev, H, self.negative_slope)
        return unignn_row_tail(Xv, skip=X0 if self.skip_sum else None, use_norm=self._use_norm(), act=act, p=p)


UNIGNN_CONVS = {'UniGAT': UniGATConv, 'UniGCN': UniGCNConv, 'UniGCN2': UniGCNConv2, 'UniGIN': UniGINConv, 'UniSAGE': UniSAGEConv}


class UniGNN(nn.Module):
    """Reference models.py:869-907: ``conv_out = Conv(nhid * nhead, nclass, heads=1)`` and ``convs = [Conv(nfeat, nhid, heads=nhead)] +
    [Conv(nhid * nhead, nhid, heads=nhead)] * (nlayer - 2)`` with ``Conv`` chosen by ``args.model_name``; input dropout, then per conv the
    activation and dropout, then ``conv_out`` and ``log_softmax``.  ``V`` / ``E``: the sorted, de-duplicated pairs of
    ``preprocessing.ConstructH_pairs``; ``args.degV`` / ``args.degE`` the scales of ``generate_norm_UniGNN``.  ``relu`` and the dropout
    ride in each conv's last launch; ``prelu`` runs unfused (conv, ``nn.PReLU``, hash dropout).  Training-mode masks are the library's
    hash dropout."""

    def __init__(self, args, nfeat, nhid, nclass, nlayer, nhead, V, E):
        super().__init__()
        if args.model_name not in UNIGNN_CONVS:
            raise ValueError(f"UniGNN: args.model_name={args.model_name!r} is not one of {tuple(sorted(UNIGNN_CONVS))}")
        Conv = UNIGNN_CONVS[args.model_name]
        self.args = args
        self.conv_out = Conv(args, nhid * nhead, nclass, heads=1, dropout=args.attn_drop)
        self.convs = nn.ModuleList(
            [Conv(args, nfeat, nhid, heads=nhead, dropout=args.attn_drop)] +
            [Conv(args, nhid * nhead, nhid, heads=nhead, dropout=args.attn_drop) for _ in range(nlayer - 2)])
        self.V = V
        self.E = E
        act = {'relu': nn.ReLU(), 'prelu': nn.PReLU()}
        self.act = act[args.activation]
        self.input_drop = nn.Dropout(args.input_drop)
        self.dropout = nn.Dropout(args.dropout)
        self._graph: Optional[UniGNNGraph] = None

    def reset_parameters(self):
        """(The reference's module has none and its driver's call fails; this one redraws every conv as its constructor does.)"""
        self.conv_out.reset_parameters()
        for conv in self.convs:
            conv.reset_parameters()
        if isinstance(self.act, nn.PReLU):
            with torch.no_grad():
                self.act.weight.fill_(0.25)

    def graph(self, x: Tensor) -> UniGNNGraph:
        """The incidence and scales on ``x``'s device, built on first sight and kept for later forwards."""
        degV, degE = _unignn_degrees(self.args)
        if self._graph is None or not self._graph.matches(self.V, self.E, degV, degE, x.device):
            if degV.shape[0] != x.shape[0]:
                raise ValueError(f"UniGNN: args.degV has {degV.shape[0]} rows, the features have {x.shape[0]}")
            self._graph = UniGNNGraph(self.V, self.E, degV, degE, x.device)
        return self._graph

    def forward(self, X):
        """``X``: the feature tensor, as the reference takes it, or a ``data`` object with ``.x``.  Returns log-probabilities."""
        X = X if torch.is_tensor(X) else X.x
        if not (X.is_cuda and X.dtype == torch.float32):
            raise AllSetHipError("the UniGNN baselines run on ROCm device fp32 tensors (no CPU path)")
        graph = self.graph(X)
        p = float(self.dropout.p) if self.training else 0.0
        X = dense.hash_dropout(X, float(self.input_drop.p), self.training)
        for conv in self.convs:
            if isinstance(self.act, nn.ReLU):
                X = conv(X, graph, act='relu', p=p)
            else:
                X = dense.hash_dropout(self.act(conv(X, graph)), p, self.training)
        X = self.conv_out(X, graph)
        return torch.log_softmax(X, dim=1)


# ---- HyperGCN ---------------------------------------------------------------------------------------------------------------------
def hypergcn_check_pairs(v_ids: Tensor, e_ids: Tensor, mediators: bool) -> None:
    """The two input families HyperGCN refuses, from the (vertex, hyperedge) pairs alone (any device, one pass at construction):
    a pair that occurs twice (the reference tells mediators from extremes by value, which makes a repeated member a third semantics
    none of its loaders produces), and -- under ``mediators`` -- a hyperedge of one member (the reference's weight 1 / (2k - 3) is -1
    there, the degree negative and the logits NaN)."""
    v, e = v_ids.reshape(-1).long(), e_ids.reshape(-1).long()
    if v.numel() == 0:
        return
    span = int(v.max()) + 1
    key = e * span + v
    uniq, counts = torch.unique(key, return_counts=True)
    if uniq.numel() != key.numel():
        first = int(uniq[counts > 1][0])
        raise ValueError(f"HyperGCN: vertex {first % span} occurs {int(counts[counts > 1][0])} times in hyperedge {first // span}; "
                         "every (vertex, hyperedge) pair must occur once")
    if mediators:
        sizes = torch.bincount(e)
        single = (sizes == 1).nonzero().reshape(-1)
        if single.numel():
            raise ValueError(f"HyperGCN with mediators: hyperedge {int(single[0])} has a single member (the reference's weight "
                             "1 / (2k - 3) is negative there and its logits are NaN); drop singleton hyperedges or run without mediators")


class HyperGraphConvolution(nn.Module):
    """Reference utils.py:11-55: ``A (H W) + bias`` with ``W`` [a, b] and ``bias`` [b] both drawn ``uniform(-1/sqrt(b), 1/sqrt(b))``,
    ``W`` first.  ``structure``: a :class:`functional.HyperGCNStructure` (``reapproximate`` False), or the vertex -> hyperedge
    ``Incidence`` when ``reapproximate``: the structure is then rebuilt from the detached ``H W`` and the projection vector ``rv`` on
    the device, with no host synchronisation.  ``rv`` defaults to the layer's own buffer ``self.rv`` [b], which
    :meth:`refresh_rv` redraws in place from a ``torch.Generator`` (the model's); the stream is torch's, not numpy's
    ``np.random.rand``, so projections differ from the reference's draw for draw while following the same distribution."""

    def __init__(self, a, b, reapproximate=True, cuda=None):
        super().__init__()
        self.a, self.b = a, b
        self.reapproximate = reapproximate
        self.W = Parameter(torch.empty(a, b))
        self.bias = Parameter(torch.empty(b))
        self.rv: Optional[Tensor] = None
        self.reset_parameters()

    def reset_parameters(self):
        std = 1. / math.sqrt(self.W.size(1))
        self.W.data.uniform_(-std, std)
        self.bias.data.uniform_(-std, std)

    def refresh_rv(self, generator: Optional[torch.Generator] = None) -> Tensor:
        """Draw ``self.rv ~ U[0, 1)^b`` in place (allocated on the parameters' device at first use): a captured graph that reads
        the buffer sees the new values at its next replay."""
        dev = self.W.device
        if self.rv is None or self.rv.device != dev:
            self.rv = torch.empty(self.b, dtype=torch.float32, device=dev)
        self.rv.uniform_(0.0, 1.0, generator=generator)
        return self.rv

    def forward(self, structure, H: Tensor, m=True, *, rv: Optional[Tensor] = None, act: Optional[str] = None, p: float = 0.0,
                fused: Optional[bool] = None) -> Tensor:
        """``act`` / ``p``: the ``relu`` and dropout the model applies next, fused into the hop's second launch."""
        if not (H.is_cuda and H.dtype == torch.float32):
            raise AllSetHipError("the HyperGCN baseline runs on ROCm device fp32 tensors (no CPU path)")
        HW = dense.linear(H, self.W.t(), None)               # H W: the [a, b] weight read transposed by the GEMM, no copy
        if self.reapproximate:
            if not isinstance(structure, Incidence):
                raise ValueError("HyperGraphConvolution(reapproximate=True) takes the vertex -> hyperedge Incidence as its structure")
            if rv is None:
                if self.rv is None or self.rv.device != HW.device:
                    if torch.cuda.is_current_stream_capturing():
                        raise RuntimeError("HyperGraphConvolution: draw the projection vector (refresh_rv) before capturing a graph")
                    self.refresh_rv()
                rv = self.rv
            structure = hypergcn_structure(HW, rv, structure, bool(m))
        elif not isinstance(structure, HyperGCNStructure):
            raise ValueError("HyperGraphConvolution(reapproximate=False) takes a functional.HyperGCNStructure")
        return hypergcn_propagate(HW, structure, self.bias, act=act, p=p, fused=fused)

    def __repr__(self):
        return self.__class__.__name__ + ' (' + str(self.a) + ' -> ' + str(self.b) + ')'


def hypergcn_widths(num_features: int, num_layers: int, num_classes: int, dname: Optional[str]) -> list:
    """Reference models.py:40-46: ``[F, 2^(L+2), 2^(L+1), ..., 2^4, C]``, the exponents two higher for ``dname == 'citeseer'``."""
    h = [num_features]
    for i in range(num_layers - 1):
        h.append(2 ** (num_layers - i + (4 if dname == 'citeseer' else 2)))
    h.append(num_classes)
    return h


class HyperGCN(nn.Module):
    """Reference models.py:29-77.  ``V``: the number of vertices; ``E``: the hypergraph as a vertex -> hyperedge ``Incidence`` or an
    int64 ``[2, nnz]`` edge list (row 0 vertex ids, row 1 hyperedge ids from 0; any device) -- not the reference's Python dict; ``X``:
    the features (kept for the signature: the fast structure is built from the ``data.x`` of the first forward, which is the same
    tensor in the driver).  ``relu`` follows every layer, the last included; dropout ``args.dropout`` every layer but the last.

    ``args.HyperGCN_fast``: ONE structure from ``data.x`` shared by all layers, built lazily on the first forward (the model is
    constructed on the host and moved to the device afterwards) or by :meth:`build_structure`.  Otherwise every layer rebuilds its
    structure from its own ``H W`` in every forward, on the device, without a host synchronisation: the forward can be captured by
    ``torch.cuda.graph``; inside a capture the projection vectors are read as they are, so call :meth:`refresh_projections`
    between replays (an eager forward does it itself).

    Projection vectors come from ``self.generator``, a ``torch.Generator`` on the model's device seeded with ``self.rv_seed`` (drawn
    from torch's global generator after the parameters, so ``torch.manual_seed`` fixes it; :meth:`seed_projections` re-seeds).  The
    stream cannot equal numpy's ``np.random.rand`` of the reference.  ``forward(data, rv=[...])`` takes explicit vectors instead.

    Refused at construction (``ValueError``): a repeated (vertex, hyperedge) pair, and a singleton hyperedge under mediators."""

    def __init__(self, V, E, X, num_features, num_layers, num_classes, args):
        super().__init__()
        self.n_vertices = int(V)
        self.m = bool(args.HyperGCN_mediators)
        self.fast = bool(args.HyperGCN_fast)
        if isinstance(E, Incidence):
            rp = E.by_dst.rowptr
            e_ids = torch.repeat_interleave(torch.arange(E.n_dst, device=rp.device), (rp[1:] - rp[:-1]).long())
            hypergcn_check_pairs(E.by_dst.col, e_ids, self.m)
            if E.n_src != self.n_vertices:
                raise ValueError(f"HyperGCN: the incidence has {E.n_src} vertices, V = {self.n_vertices}")
            self._inc, self._pairs = E, None
        else:
            if not torch.is_tensor(E) or E.dim() != 2 or E.shape[0] != 2 or E.dtype.is_floating_point:
                raise ValueError("HyperGCN: E is the vertex -> hyperedge Incidence or an integer [2, nnz] edge list")
            if E.numel() and (int(E[0].min()) < 0 or int(E[0].max()) >= self.n_vertices or int(E[1].min()) < 0):
                raise ValueError(f"HyperGCN: vertex ids must lie in [0, {self.n_vertices}) and hyperedge ids start at 0")
            hypergcn_check_pairs(E[0], E[1], self.m)
            self._inc, self._pairs = None, E.to(torch.int64)
        h = hypergcn_widths(num_features, num_layers, num_classes, getattr(args, 'dname', None))
        self.layers = nn.ModuleList([HyperGraphConvolution(h[i], h[i + 1], not self.fast) for i in range(num_layers)])
        self.do, self.l = args.dropout, num_layers
        self.structure: Optional[HyperGCNStructure] = None       # fast mode: built on the first forward
        self.rv_seed = int(torch.randint(0, 2 ** 62, (1,)))
        self.generator: Optional[torch.Generator] = None

    def reset_parameters(self):
        for layer in self.layers:
            layer.reset_parameters()

    # ---- projections --------------------------------------------------------------------------------------------------------------
    def seed_projections(self, seed: int) -> None:
        self.rv_seed = int(seed)
        self.generator = None

    def _generator(self, device) -> torch.Generator:
        if self.generator is None or self.generator.device != device:
            self.generator = torch.Generator(device=device)
            self.generator.manual_seed(self.rv_seed)
        return self.generator

    def refresh_projections(self) -> None:
        """Redraw every layer's projection vector in place (re-approximating mode; nothing to do in fast mode)."""
        if self.fast:
            return
        gen = self._generator(self.layers[0].W.device)
        for layer in self.layers:
            layer.refresh_rv(gen)

    # ---- structure ----------------------------------------------------------------------------------------------------------------
    def incidence(self, device) -> Incidence:
        if self._inc is None or self._inc.device != device:
            if self._pairs is None:
                raise AllSetHipError(f"HyperGCN: the incidence lives on {self._inc.device}, the features on {device}")
            n_e = int(self._pairs[1].max()) + 1 if self._pairs.numel() else 0
            self._inc = Incidence.from_edge_index(self._pairs.to(device).contiguous(), n_src=self.n_vertices, n_dst=n_e)
        return self._inc

    def build_structure(self, x: Tensor, rv: Optional[Tensor] = None) -> HyperGCNStructure:
        """Fast mode's one structure, from ``x`` and ``rv`` [x.shape[1]] (drawn from the model's generator when None)."""
        if rv is None:
            rv = torch.empty(x.shape[1], dtype=torch.float32, device=x.device).uniform_(0.0, 1.0, generator=self._generator(x.device))
        self.structure = hypergcn_structure(x, rv, self.incidence(x.device), self.m)
        return self.structure

    def forward(self, data, rv=None):
        """``rv``: explicit projection vectors, one [width of layer i's output] per layer (re-approximating mode only)."""
        H = data.x
        if not (H.is_cuda and H.dtype == torch.float32):
            raise AllSetHipError("the HyperGCN baseline runs on ROCm device fp32 tensors (no CPU path)")
        if H.shape[0] != self.n_vertices:
            raise ValueError(f"HyperGCN: data.x has {H.shape[0]} rows, V = {self.n_vertices}")
        if self.fast:
            if rv is not None:
                raise ValueError("HyperGCN(fast): the one projection vector goes to build_structure(x, rv)")
            if self.structure is None or self.structure.inc.device != H.device:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("HyperGCN(fast): run one forward (or build_structure) before capturing a graph")
                self.build_structure(H)
            structure = self.structure
        else:
            structure = self.incidence(H.device)
            if rv is None and not torch.cuda.is_current_stream_capturing():
                self.refresh_projections()
        p = float(self.do) if self.training else 0.0
        for i, hidden in enumerate(self.layers):
            H = hidden(structure, H, self.m, rv=None if rv is None else rv[i], act='relu', p=p if i < self.l - 1 else 0.0)
        return H
