"""The heterogeneous mode of the reference's HAN program (``src/DGL_HAN/main.py --hetero``, ``model_hetero.py``) on the HIP path.

In that mode HAN receives ONE typed graph and a list of metapaths (lists of edge types) and derives the per-metapath graphs itself
with ``dgl.metapath_reachable_graph``.  Here: :class:`HeteroGraph` (the typed graph: per-relation CSR on the device),
:func:`metapath_reachable_graph` (DGL 0.7.1's semantics as a left-to-right chain of boolean sparse products, ``csrc/metapath.hip`` --
device memory proportional to the result, not to the candidate pairs), and the model classes with ``model_hetero.py``'s names,
constructor signatures, creation order and ``state_dict`` keys.  The hops are ``han.py``'s: ``functional.han_gat_propagate`` writing
its column block of the stacked buffer, ``functional.semantic_attention``.

What differs from ``han.py``'s graphs: no self-loop is appended and a node without an incoming edge is allowed (the reference builds
its ``GATConv`` with ``allow_zero_in_degree=True``); such a node's output is ``elu(bias)`` and only ``bias`` receives its gradient.

Driver: ``python -m allset_amd.han --hetero`` (``--dataset synthetic``: ``synthetic.acm_like_hetero``; DGL's ACMRaw download is not
read here)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, dense, han, ops
from .incidence import Incidence

Tensor = torch.Tensor
INT32_MAX = 2 ** 31 - 1
CanonicalEType = Tuple[str, str, str]


class HeteroGraph:
    """A typed directed graph.  ``edges`` maps ``(srctype, etype, dsttype)`` to a pair ``(src ids, dst ids)`` of int64 tensors -- the
    first argument of ``dgl.heterograph``; ``num_nodes`` maps a node type to its count (default, as in DGL: the largest id of the
    type over all relations, plus one).  Ids are checked here, once; the per-relation CSR (rows = sources, int32, on the device) is
    built on first use."""

    def __init__(self, edges: Dict[CanonicalEType, Tuple[Tensor, Tensor]], num_nodes: Optional[Dict[str, int]] = None):
        if not isinstance(edges, dict) or not edges:
            raise ValueError("HeteroGraph: edges must be a non-empty dict {(srctype, etype, dsttype): (src, dst)}")
        self._edges: Dict[CanonicalEType, Tuple[Tensor, Tensor]] = {}
        extent: Dict[str, int] = {}
        names: Dict[str, CanonicalEType] = {}
        for rel, pair in edges.items():
            if not (isinstance(rel, tuple) and len(rel) == 3 and all(isinstance(s, str) for s in rel)):
                raise ValueError(f"HeteroGraph: relation key {rel!r} is not a (srctype, etype, dsttype) triple of strings")
            if not (isinstance(pair, (tuple, list)) and len(pair) == 2 and all(torch.is_tensor(t) for t in pair)):
                raise ValueError(f"HeteroGraph: relation {rel}: expected a pair (src, dst) of id tensors")
            src, dst = pair
            if src.dtype != torch.int64 or dst.dtype != torch.int64 or src.dim() != 1 or dst.dim() != 1:
                raise ValueError(f"HeteroGraph: relation {rel}: ids must be 1-D int64 tensors (got {src.dtype} {tuple(src.shape)}, "
                                 f"{dst.dtype} {tuple(dst.shape)})")
            if src.numel() != dst.numel():
                raise ValueError(f"HeteroGraph: relation {rel}: {src.numel()} source ids but {dst.numel()} target ids")
            if src.numel() > INT32_MAX:
                raise ValueError(f"HeteroGraph: relation {rel} has {src.numel()} edges: edge slots are int32 (at most {INT32_MAX})")
            if src.device != dst.device:
                raise ValueError(f"HeteroGraph: relation {rel}: ids on different devices")
            if rel[1] in names:
                raise ValueError(f"HeteroGraph: edge type {rel[1]!r} names two relations, {names[rel[1]]} and {rel}")
            names[rel[1]] = rel
            for ntype, ids in ((rel[0], src), (rel[2], dst)):
                lo, hi = (int(ids.min()), int(ids.max())) if ids.numel() else (0, -1)
                if lo < 0:
                    raise ValueError(f"HeteroGraph: relation {rel}: negative {ntype!r} id {lo}")
                extent[ntype] = max(extent.get(ntype, 0), hi + 1)
            self._edges[rel] = (src.contiguous(), dst.contiguous())
        self._num_nodes = dict(extent)
        if num_nodes is not None:
            for ntype, n in num_nodes.items():
                if int(n) < extent.get(ntype, 0):
                    raise ValueError(f"HeteroGraph: num_nodes[{ntype!r}] = {n} but ids of that type reach {extent[ntype] - 1}")
                self._num_nodes[ntype] = int(n)
        for ntype, n in self._num_nodes.items():
            if n > INT32_MAX:
                raise ValueError(f"HeteroGraph: {n} nodes of type {ntype!r}: node ids are int32 on the device (at most {INT32_MAX})")
        self._names = names
        self._csr: Dict[CanonicalEType, ops.CSR] = {}

    @property
    def ntypes(self) -> List[str]:
        return sorted(self._num_nodes)

    @property
    def canonical_etypes(self) -> List[CanonicalEType]:
        return list(self._edges)

    def number_of_nodes(self, ntype: str) -> int:
        if ntype not in self._num_nodes:
            raise ValueError(f"HeteroGraph: unknown node type {ntype!r} (known: {self.ntypes})")
        return self._num_nodes[ntype]

    def to_canonical_etype(self, etype) -> CanonicalEType:
        """``etype`` (a name or a triple) -> ``(srctype, etype, dsttype)``; ``ValueError`` for one this graph does not have."""
        if isinstance(etype, tuple):
            if etype not in self._edges:
                raise ValueError(f"HeteroGraph: unknown relation {etype!r} (known: {self.canonical_etypes})")
            return etype
        if etype not in self._names:
            raise ValueError(f"HeteroGraph: unknown edge type {etype!r} (known: {sorted(self._names)})")
        return self._names[etype]

    def edges(self, etype) -> Tuple[Tensor, Tensor]:
        return self._edges[self.to_canonical_etype(etype)]

    def csr(self, etype) -> ops.CSR:
        """The relation's CSR with rows = source ids (duplicate edges kept), built on the device once."""
        rel = self.to_canonical_etype(etype)
        if rel not in self._csr:
            src, dst = self._edges[rel]
            _lib.require_device(src, dst)
            self._csr[rel] = ops.csr_build(src, dst, 0, 0, self._num_nodes[rel[0]], self._num_nodes[rel[2]])
        return self._csr[rel]


class ReachableGraph:
    """What :func:`metapath_reachable_graph` returns: the edges ``src -> dst`` (int64, row-major: sources ascending, targets ascending
    within a source, one edge per pair) from ``n_src`` nodes of ``srctype`` to ``n_dst`` nodes of ``dsttype``, in both CSR
    orientations with the attributes the hop kernels read from a ``han.MetapathGraph`` -- ``rowptr`` / ``col`` / ``perm``
    (target-major), ``rowptrT`` / ``colT`` / ``slotT`` (source-major), ``n`` (= ``n_dst``), ``nnz``.  Unlike ``han.MetapathGraph`` a
    target without an incoming edge is allowed (``zero_in_degree`` says whether there is one)."""

    def __init__(self, src: Tensor, dst: Tensor, n_src: int, n_dst: int, srctype: str = "_N", dsttype: str = "_N"):
        if src.numel() > INT32_MAX:
            raise ValueError(f"metapath graph with {src.numel()} edges: edge slots are int32 (at most {INT32_MAX})")
        _lib.require_device(src, dst)
        self.srctype, self.dsttype = srctype, dsttype
        self.n_src, self.n_dst, self.n, self.nnz = int(n_src), int(n_dst), int(n_dst), int(src.numel())
        self.src, self.dst = src.contiguous(), dst.contiguous()
        inc = Incidence.from_edge_index(torch.stack([self.src, self.dst]), n_src=self.n_src, n_dst=self.n_dst)
        self.rowptr, self.col, self.perm = inc.by_dst.rowptr, inc.by_dst.col, inc.by_dst.perm
        self.rowptrT, self.colT = inc.by_src.rowptr, inc.by_src.col
        self.slotT = inc.pos_dst_of_src()
        self.zero_in_degree = bool(self.n_dst > 0 and bool((self.rowptr[1:] == self.rowptr[:-1]).any()))


def _check_metapath(g: HeteroGraph, metapath: Sequence) -> List[CanonicalEType]:
    if isinstance(metapath, str) or len(metapath) < 1:
        raise ValueError(f"metapath must be a non-empty list of edge types, got {metapath!r}")
    rels = [g.to_canonical_etype(e) for e in metapath]
    for i in range(len(rels) - 1):
        if rels[i][2] != rels[i + 1][0]:
            raise ValueError(f"metapath {list(metapath)!r}: step {i} ({rels[i][1]!r}) ends on {rels[i][2]!r} but step {i + 1} "
                             f"({rels[i + 1][1]!r}) starts from {rels[i + 1][0]!r}")
    return rels


def metapath_reachable_csr(g: HeteroGraph, metapath: Sequence) -> Tuple[Tensor, Tensor, CanonicalEType]:
    """``(rowptr int32[n_first + 1], col int32[nnz], (srctype, '_E', dsttype))``: the pattern of the product of the metapath's
    adjacency matrices, columns strictly increasing within each row."""
    rels = _check_metapath(g, metapath)
    a = g.csr(rels[0])
    rowptr, col = a.rowptr, a.col
    if len(rels) == 1:                                        # binarise and sort the single relation: its product with the identity
        n = g.number_of_nodes(rels[0][2])
        eye = torch.arange(n + 1, dtype=torch.int32, device=rowptr.device)
        return (*ops.spgemm_bool(rowptr, col, eye, eye[:n].contiguous(), n), (rels[0][0], "_E", rels[0][2]))
    for rel in rels[1:]:
        b = g.csr(rel)
        rowptr, col = ops.spgemm_bool(rowptr, col, b.rowptr, b.col, g.number_of_nodes(rel[2]))
    return rowptr, col, (rels[0][0], "_E", rels[-1][2])


def metapath_reachable_edges(g: HeteroGraph, metapath: Sequence) -> Tuple[Tensor, Tensor, str, str]:
    """``(src, dst, srctype, dsttype)``: the reachable pairs as int64 edge lists in row-major order (sources ascending, targets
    ascending within a source)."""
    rowptr, col, (srctype, _, dsttype) = metapath_reachable_csr(g, metapath)
    n_src = g.number_of_nodes(srctype)
    deg = (rowptr[1:] - rowptr[:-1]).long()
    src = torch.repeat_interleave(torch.arange(n_src, dtype=torch.int64, device=col.device), deg, output_size=int(col.numel()))
    return src, col.long(), srctype, dsttype


def metapath_reachable_graph(g: HeteroGraph, metapath: Sequence) -> ReachableGraph:
    """``dgl.metapath_reachable_graph`` (DGL 0.7.1): an edge ``u -> w`` exactly when some walk from ``u`` follows the metapath's edge
    types in order and ends in ``w``; ``u`` of the first relation's source type, ``w`` of the last one's destination type; one edge
    per pair, no self-loop added or removed.  Any length >= 1.  ``ValueError`` for an unknown edge type or when a step does not
    start where the previous one ended."""
    src, dst, srctype, dsttype = metapath_reachable_edges(g, metapath)
    return ReachableGraph(src, dst, g.number_of_nodes(srctype), g.number_of_nodes(dsttype), srctype, dsttype)


# --------------------------------------------------------------------------------------------------
# model (reference DGL_HAN/model_hetero.py)
# --------------------------------------------------------------------------------------------------

class GATConv(han.GATConv):
    """``han.GATConv`` that accepts ``allow_zero_in_degree=True`` (how ``model_hetero.py`` builds it).  Without it a graph with a
    0-in-degree node raises at the forward, as DGL's does."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0., negative_slope=0.2, residual=False,
                 activation=None, allow_zero_in_degree=False, bias=True):
        super().__init__(in_feats, out_feats, num_heads, feat_drop, attn_drop, negative_slope, residual, activation, False, bias)
        self._allow_zero_in_degree = bool(allow_zero_in_degree)

    def forward(self, graph, feat: Tensor, out: Optional[Tensor] = None, block: int = 0) -> Tensor:
        if not self._allow_zero_in_degree and getattr(graph, "zero_in_degree", False):
            raise ValueError("There are 0-in-degree nodes in the graph, output for those nodes will be invalid. Construct the "
                             "GATConv with allow_zero_in_degree=True to get elu(bias) for them.")
        return super().forward(graph, feat, out=out, block=block)


SemanticAttention = han.SemanticAttention


class HANLayer(nn.Module):
    """``meta_paths``: a list of metapaths, each a list of edge types.  ``forward(g, h)``: ``g`` a :class:`HeteroGraph`, ``h`` the
    features of the node type every metapath starts from and ends on.  The reachable graphs are derived once per graph object."""

    def __init__(self, meta_paths, in_size, out_size, layer_num_heads, dropout):
        super().__init__()
        self.gat_layers = nn.ModuleList()
        for _ in range(len(meta_paths)):
            self.gat_layers.append(GATConv(in_size, out_size, layer_num_heads, dropout, dropout, activation=F.elu,
                                           allow_zero_in_degree=True))
        self.semantic_attention = SemanticAttention(in_size=out_size * layer_num_heads)
        self.meta_paths = list(tuple(meta_path) for meta_path in meta_paths)
        self._cached_graph = None
        self._cached_coalesced_graph = {}

    def reachable_graphs(self, g: HeteroGraph) -> List[ReachableGraph]:
        if self._cached_graph is None or self._cached_graph is not g:
            built = {}
            for meta_path in self.meta_paths:
                rg = metapath_reachable_graph(g, meta_path)
                if rg.srctype != rg.dsttype:
                    raise ValueError(f"HANLayer: metapath {list(meta_path)!r} leads from {rg.srctype!r} to {rg.dsttype!r}; the layer's "
                                     "input has one row per node of ONE type, so a metapath must end on the type it starts from")
                built[meta_path] = rg
            self._cached_graph = g
            self._cached_coalesced_graph = built
        return [self._cached_coalesced_graph[mp] for mp in self.meta_paths]

    def forward(self, g: HeteroGraph, h: Tensor) -> Tensor:
        gs = self.reachable_graphs(g)
        M = len(gs)
        d = self.gat_layers[0]._num_heads * self.gat_layers[0]._out_feats
        z = torch.empty((h.shape[0], M * d), dtype=torch.float32, device=h.device)      # the reference's torch.stack(..., dim=1)
        for i, rg in enumerate(gs):
            z = self.gat_layers[i](rg, h, out=z, block=i)
        return self.semantic_attention(z.view(h.shape[0], M, d))


class HAN(nn.Module):
    def __init__(self, meta_paths, in_size, hidden_size, out_size, num_heads, dropout):
        super().__init__()
        self.layers = nn.ModuleList()
        self.layers.append(HANLayer(meta_paths, in_size, hidden_size, num_heads[0], dropout))
        for l in range(1, len(num_heads)):
            self.layers.append(HANLayer(meta_paths, hidden_size * num_heads[l - 1], hidden_size, num_heads[l], dropout))
        self.predict = nn.Linear(hidden_size * num_heads[-1], out_size)

    def forward(self, g: HeteroGraph, h: Tensor) -> Tensor:
        for gnn in self.layers:
            h = gnn(g, h)
        return dense.linear(h, self.predict.weight, self.predict.bias)


# --------------------------------------------------------------------------------------------------
# driver pieces (reference DGL_HAN/main.py with --hetero; the loop itself is han.main's)
# --------------------------------------------------------------------------------------------------

META_PATHS = [['pa', 'ap'], ['pf', 'fp']]


def load_data(args: dict):
    """``(g, features, labels, num_classes)`` on ``args['device']`` for ``--hetero``."""
    if args['dataset'] != 'synthetic':
        raise FileNotFoundError(f"dataset {args['dataset']!r} is not available to --hetero: the reference downloads DGL's ACM.mat "
                                "(ACMRaw), which is not distributed with it and is not read here; use --dataset synthetic")
    from .synthetic import acm_like_hetero
    d = acm_like_hetero(seed=args['seed'], device=args['device'])
    return HeteroGraph(d.edges, d.num_nodes), d.features, d.labels, d.num_classes


def make_model(args: dict, in_size: int, num_classes: int) -> HAN:
    return HAN(meta_paths=META_PATHS, in_size=in_size, hidden_size=args['hidden_units'], out_size=num_classes,
               num_heads=args['num_heads'], dropout=args['dropout'])
