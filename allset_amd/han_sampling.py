"""Mini-batch HAN of the reference's results table (``src/DGL_HAN/train_sampling.py``) on the HIP path.

The reference samples on CPU ``DataLoader`` workers through DGL: per seed ``k`` metapath random walks
(``RandomWalkNeighborSampler(num_traversals=1, termination_prob=0, num_random_walks=k, num_neighbors=k)``), the distinct endpoints as
neighbours, self-loops removed and exactly one added back, ``dgl.to_block`` with the seeds first.  Here the incidence, the features and
the labels stay on the device and the sampler is three HIP kernels (``csrc/han_sample.hip``: the walk, the per-seed rows, the
relabelling) around one torch sort; the GAT hop runs over the bipartite block (``functional.han_block_propagate``).

Node ids are the "appended" space full-batch HAN uses: vertices ``0..n_v-1``, hyperedges ``n_v..n_v+n_e-1``.  ``['Vs_E', 'E_Vs']`` (VEV)
leaves only vertex ids, ``['Es_V', 'V_Es']`` (EVE) only hyperedge ids; a walk from any other node terminates and contributes nothing, so
for the labelled seeds (vertices) the EVE block is the self-loops alone -- the reference's behaviour, kept.

Orderings chosen here (DGL's are hash-table orders): a target's neighbours ascending by global id with the self-loop last; the block's
source nodes = the seeds in the given order, then the other distinct nodes ascending.  Random numbers are counter-based, keyed on
``(seed, step counter, metapath, global seed node, walk, hop)``: a node's neighbours do not depend on the batch it is in.

A typed graph (the reference's ``ACMRaw`` branch, metapaths of edge types such as ``[['pa', 'ap'], ['pf', 'fp']]``) is sampled through
:class:`TypedMetapathWalker` over a ``han_hetero.HeteroGraph``: the walk follows the metapath's chain of relation CSRs (any length up
to ``ops.HAN_MAX_HOPS``, duplicate edges kept) in the ids of the node type every metapath starts from and ends on; everything after
the walk is the same code.  ``--hetero`` runs it.

``HANSampler.sample_blocks_fixed`` builds the same blocks at a capacity that depends on ``(B, k)`` alone and never reads a size back
(:class:`FixedBlock`); :class:`GraphedSampledStep` replays one whole training step -- sampler included -- as one hipGraph
(``--fixed_blocks`` / ``--graph_step``).

Reference quirks kept: ``evaluate`` samples ``2 k`` walks and returns the LAST batch's loss (which ``EarlyStopping`` then consumes);
``HAN.forward`` hands the same blocks to every layer, so only ``len(num_heads) == 1`` can work -- more raises ``ValueError``.
"""
from __future__ import annotations

import argparse
import time
from types import SimpleNamespace
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, dense, han_hetero, ops
from .functional import han_block_propagate, semantic_attention
from .han import EarlyStopping, SemanticAttention, _first, node_features, rand_train_test_idx, score
from .han_hetero import META_PATHS, CanonicalEType, HeteroGraph, _check_metapath
from .incidence import Incidence

Tensor = torch.Tensor
INT32_MAX = 2 ** 31 - 1
METAPATHS = {('Vs_E', 'E_Vs'): 0, ('Es_V', 'V_Es'): 1}
DEFAULT_METAPATHS = [['Vs_E', 'E_Vs'], ['Es_V', 'V_Es']]


def metapath_index(metapath) -> int:
    """0 for VEV (``['Vs_E', 'E_Vs']``, ``'VEV'`` or 0), 1 for EVE (``['Es_V', 'V_Es']``, ``'EVE'`` or 1)."""
    if isinstance(metapath, str) and metapath in ('VEV', 'EVE'):
        return 0 if metapath == 'VEV' else 1
    if isinstance(metapath, (int, np.integer)) and int(metapath) in (0, 1):
        return int(metapath)
    try:
        return METAPATHS[tuple(metapath)]
    except (KeyError, TypeError):
        raise ValueError(f"unknown metapath {metapath!r}: ['Vs_E', 'E_Vs'] (VEV) and ['Es_V', 'V_Es'] (EVE) are built") from None


# --------------------------------------------------------------------------------------------------
# sampler
# --------------------------------------------------------------------------------------------------

class MetapathWalker:
    """The binarised (vertex, hyperedge) incidence of ``data`` as both CSRs on the device, built once: ``v2e`` (row = vertex) and
    ``e2v`` (row = hyperedge) are the two orientations of one :class:`Incidence`.  ``data.edge_index`` holds the incidences with
    hyperedge ids starting at ``e_base``; ``data.n_x`` vertices, ``data.num_hyperedges`` hyperedges."""

    def __init__(self, data, e_base: int = 0):
        n_v, n_e = _first(data.n_x), _first(data.num_hyperedges)
        ei = data.edge_index
        _lib.require_device(ei)
        v, e = ei[0], ei[1] - int(e_base)
        if ei.numel() and (int(v.min()) < 0 or int(v.max()) >= n_v or int(e.min()) < 0 or int(e.max()) >= n_e):
            raise ValueError(f"MetapathWalker: incidences outside {n_v} vertices x {n_e} hyperedges (hyperedge ids start at e_base = {e_base})")
        if n_v + n_e > INT32_MAX:
            raise ValueError(f"MetapathWalker: {n_v + n_e} nodes: node ids are int32")
        key = torch.unique(v * max(n_e, 1) + e)                       # binarise (the reference's .nonzero(): duplicates count once)
        pairs = torch.stack([key // max(n_e, 1), key % max(n_e, 1)])
        inc = Incidence.from_edge_index(pairs, n_src=n_v, n_dst=n_e)
        self.n_v, self.n_e, self.n = n_v, n_e, n_v + n_e
        self.v2e, self.e2v = inc.by_src, inc.by_dst
        self.device = ei.device

    def orientation(self, mp: int):
        """``(CSR A, CSR B, id_base)`` of metapath ``mp``."""
        return (self.v2e, self.e2v, 0) if mp == 0 else (self.e2v, self.v2e, self.n_v)


class TypedMetapathWalker:
    """A typed graph for the sampler: metapaths are lists of ``g``'s edge types (names or canonical triples), walked over the chain of
    ``g.csr(etype)`` -- duplicate edges kept, so a duplicated edge is twice as likely, as in DGL's multigraph walk.  The sampler builds a
    homogeneous neighbour graph on ONE node type (DGL's ``RandomWalkNeighborSampler``): every metapath starts from and ends on it.  That
    type is fixed by the first metapaths the walker is used with (``ntype``, and ``n`` = its node count: the seeds' id range); a
    walker serves one node type, a second one over the same graph shares its CSRs."""

    def __init__(self, g: HeteroGraph):
        if not isinstance(g, HeteroGraph):
            raise TypeError(f"TypedMetapathWalker: a han_hetero.HeteroGraph is required (got {type(g).__name__})")
        self.g = g
        self.device = g.edges(g.canonical_etypes[0])[0].device
        self.ntype: Optional[str] = None
        self.n: Optional[int] = None

    def resolve(self, metapath) -> List[CanonicalEType]:
        """The metapath's relations.  Host only; ``ValueError`` for an empty metapath, an unknown edge type, a step that does not start
        where the previous one ended, more than ``ops.HAN_MAX_HOPS`` steps, or a metapath that does not end on the type it starts
        from (its endpoints would be taken for ids of the seeds' type)."""
        rels = _check_metapath(self.g, metapath)
        if len(rels) > ops.HAN_MAX_HOPS:
            raise ValueError(f"metapath {list(metapath)!r} has {len(rels)} steps: the walk kernel is built for at most HAN_MAX_HOPS = "
                             f"{ops.HAN_MAX_HOPS}")
        if rels[0][0] != rels[-1][2]:
            raise ValueError(f"metapath {list(metapath)!r} leads from {rels[0][0]!r} to {rels[-1][2]!r}: the sampled neighbours are nodes "
                             "of the seeds' type, so a metapath must end on the type it starts from")
        return rels

    def bind(self, metapath_list) -> List[List[CanonicalEType]]:
        """Every metapath resolved; all must start from one node type, which becomes (or must be) the walker's."""
        chains = [self.resolve(m) for m in metapath_list]
        heads = sorted({rels[0][0] for rels in chains})
        if len(heads) != 1:
            raise ValueError(f"metapaths {[list(m) for m in metapath_list]!r} start from {len(heads)} node types {heads}: the seeds of a "
                             "batch are ids of ONE type")
        if self.ntype is not None and self.ntype != heads[0]:
            raise ValueError(f"this walker samples {self.ntype!r} nodes; metapaths from {heads[0]!r} need a TypedMetapathWalker of "
                             "their own")
        self.ntype, self.n = heads[0], self.g.number_of_nodes(heads[0])
        return chains

    def chain(self, rels: Sequence[CanonicalEType]) -> List[ops.CSR]:
        return [self.g.csr(rel) for rel in rels]


def _walk(walker, mp: int, rels, s32: Tensor, k: int, seed: int, counter, counter_add: int = 0) -> Tensor:
    """int32[B, k] endpoints of metapath ``mp``: over ``rels`` (a typed walker's relation chain) or, ``rels`` None, the incidence.
    ``counter``: an int, or a 1-element device tensor (plus ``counter_add``) the walk kernel reads."""
    if rels is not None:
        return ops.han_walk_typed(mp, walker.chain(rels), s32, k, seed, counter, counter_add)
    a, b, base = walker.orientation(mp)
    return ops.han_walk(mp, a, b, base, s32, k, seed, counter, counter_add)


def _seeds_on_device(walker, seeds, check_dups: bool) -> Tensor:
    """int32[B] on the walker's device.  A host list / CPU tensor is range-checked (and checked for duplicates) on the host for free;
    a device tensor is taken as it is -- out-of-range ids there are nodes without out-edges to the walk."""
    if torch.is_tensor(seeds) and seeds.is_cuda:
        return seeds.to(torch.int32).contiguous().view(-1)
    host = np.asarray(seeds.cpu() if torch.is_tensor(seeds) else seeds).reshape(-1)
    if host.size and host.dtype.kind not in "iu":
        raise ValueError(f"seeds must be integer node ids (got {host.dtype})")
    host = host.astype(np.int64)
    if host.size and (host.min() < 0 or host.max() >= walker.n):
        raise ValueError(f"seeds outside [0, {walker.n}): {int(host.min())}..{int(host.max())}")
    if check_dups and np.unique(host).size != host.size:
        raise ValueError("duplicate seeds: a block's target nodes are distinct (dgl.to_block raises too)")
    return torch.from_numpy(host.astype(np.int32)).to(walker.device)


def random_walk_endpoints(walker, metapath, seeds, num_walks: int, seed: int, counter: int, index: int = 0) -> Tensor:
    """The raw walks: int64[B, num_walks] endpoints in global ids, -1 for a walk that terminated (a seed without out-edges in this
    metapath).  A pure function of its arguments.  With a :class:`TypedMetapathWalker`, ``metapath`` is a list of edge types and
    ``index`` its position in the sampler's metapath list (the metapath index of the random-number key)."""
    typed = isinstance(walker, TypedMetapathWalker)
    if typed:
        if not 0 <= int(index) < 256:
            raise ValueError(f"index must be in [0, 256) (got {index})")
        mp, rels = int(index), walker.bind([metapath])[0]
    else:
        mp, rels = metapath_index(metapath), None
    if not 1 <= int(num_walks) <= ops.HAN_MAX_WALKS:
        raise ValueError(f"num_walks must be in [1, {ops.HAN_MAX_WALKS}] (got {num_walks})")
    s32 = _seeds_on_device(walker, seeds, check_dups=False)
    return _walk(walker, mp, rels, s32, int(num_walks), seed, counter).long()


class Block:
    """A bipartite block, DGL's ``to_block`` result: ``n_src`` source nodes (``src_ids`` int64 global ids, the ``n_dst`` targets
    first) and edges source -> target in block-local ids.  ``src`` / ``dst`` int64[nnz]: the edge list; ``rowptr`` / ``col``:
    target-major CSR (a slot there is the edge's identity for the attention dropout), ``perm``: slot -> edge-list position;
    ``rowptrT`` / ``colT`` / ``slotT``: source-major CSR and the target-major slot of each of its entries, as in
    ``han.MetapathGraph``."""

    def __init__(self, n_dst, n_src, src_ids, src, dst, rowptr, col, perm, rowptrT, colT, slotT):
        self.n_dst, self.n_src, self.nnz = int(n_dst), int(n_src), int(col.numel())
        self.src_ids, self.src, self.dst = src_ids, src, dst
        self.rowptr, self.col, self.perm = rowptr, col, perm
        self.rowptrT, self.colT, self.slotT = rowptrT, colT, slotT

    @staticmethod
    def from_edges(src: Tensor, dst: Tensor, n_src: int, n_dst: int, src_ids: Optional[Tensor] = None) -> "Block":
        """From a block-local edge list on the device (any order, duplicates kept)."""
        _lib.require_device(src, dst)
        if n_dst > n_src:
            raise ValueError(f"a block's targets are its first source nodes: n_dst = {n_dst} > n_src = {n_src}")
        src, dst = src.long().contiguous(), dst.long().contiguous()
        inc = Incidence.from_edge_index(torch.stack([src, dst]), n_src=n_src, n_dst=n_dst)
        if src_ids is None:
            src_ids = torch.arange(n_src, dtype=torch.int64, device=src.device)
        return Block(n_dst, n_src, src_ids, src, dst, inc.by_dst.rowptr, inc.by_dst.col, inc.by_dst.perm, inc.by_src.rowptr,
                     inc.by_src.col, inc.pos_dst_of_src())

    def srcdata_nid(self) -> Tensor:
        return self.src_ids


class FixedBlock(Block):
    """A :class:`Block` whose Python-side shape depends on ``(B, k)`` alone, built without a host read-back
    (:meth:`HANSampler.sample_blocks_fixed`): ``n_dst = B`` and ``n_src = nnz = B * (k + 1)``, the capacity that cannot overflow (at
    most ``B * k`` distinct non-seed nodes, at most ``k + 1`` slots per target).  The real sizes stay on the device in ``sizes``,
    int32[2] = ``{nnz_real, n_extra}`` (``n_src_real = B + n_extra``); :meth:`exact` reads them back and returns the ordinary block --
    for tests and debugging, never for the training path.

    Padding contract (what the hop kernels and a feature gather rely on):

    * ``rowptr[B] == nnz_real``: no target row contains a slot ``>= nnz_real``;
    * ``rowptrT[j] == nnz_real`` for every ``j >= n_src_real``: padded source rows are EMPTY rows of the source-major CSR (the hop's
      backward writes exact zeros for them);
    * every entry of ``col``, ``colT``, ``slotT``, ``dst`` and ``src_ids`` is in range over the full capacity: padding is 0, and the
      first seed's id in ``src_ids``, so ``features[src_ids]`` is a valid gather;
    * the real part is :meth:`HANSampler.sample_blocks`'s block entry for entry: ``rowptr``, ``col[:nnz]``, ``dst[:nnz]``,
      ``src_ids[:n_src]``, ``rowptrT[:n_src + 1]``, ``colT[:nnz]``, ``slotT[:nnz]``; ``perm`` is the identity.

    ``src`` / ``dst`` (the int64 edge list) and ``perm`` are made on first use: the model reads neither."""

    def __init__(self, B: int, k: int, src_ids: Tensor, rowptr: Tensor, col: Tensor, dst32: Tensor, rowptrT: Tensor, colT: Tensor,
                 slotT: Tensor, sizes: Tensor):
        cap = FixedBlock.capacity(B, k)
        self.n_dst, self.n_src, self.nnz, self.k = int(B), cap, cap, int(k)
        self.src_ids, self.rowptr, self.col, self.dst32 = src_ids, rowptr, col, dst32
        self.rowptrT, self.colT, self.slotT, self.sizes = rowptrT, colT, slotT, sizes

    @staticmethod
    def capacity(B: int, k: int) -> int:
        """``B * (k + 1)``: source rows and slots of a fixed block of ``B`` targets with ``k`` walks each."""
        return int(B) * (int(k) + 1)

    @property
    def src(self) -> Tensor:
        return self.col.long()

    @property
    def dst(self) -> Tensor:
        return self.dst32.long()

    @property
    def perm(self) -> Tensor:
        return torch.arange(self.nnz, dtype=torch.int32, device=self.col.device)

    def exact(self) -> Block:
        """The ordinary :class:`Block` of the real part.  ONE host read-back: tests and debugging only."""
        nnz, n_extra = (int(v) for v in self.sizes.tolist())
        n_src = self.n_dst + n_extra
        col, dst = self.col[:nnz], self.dst32[:nnz]
        return Block(self.n_dst, n_src, self.src_ids[:n_src], col.long(), dst.long(), self.rowptr, col,
                     torch.arange(nnz, dtype=torch.int32, device=col.device), self.rowptrT[:n_src + 1], self.colT[:nnz],
                     self.slotT[:nnz])


class HANSampler:
    """``HANSampler(g, metapath_list, num_neighbors)`` of the reference with the device-resident walker in ``g``'s place and an
    explicit ``seed``.  Every :meth:`sample_blocks` call takes the next step counter (or the one given).  With a
    :class:`TypedMetapathWalker`, ``metapath_list`` holds lists of edge types and a metapath's index is its position in the list."""

    def __init__(self, walker, metapath_list, num_neighbors: int, seed: int = 0):
        if not 1 <= int(num_neighbors) <= ops.HAN_MAX_WALKS:
            raise ValueError(f"num_neighbors must be in [1, {ops.HAN_MAX_WALKS}] (got {num_neighbors}): the walk kernel is built for "
                             f"at most {ops.HAN_MAX_WALKS} walks per seed")
        self.walker, self.num_neighbors, self.seed = walker, int(num_neighbors), int(seed)
        if isinstance(walker, TypedMetapathWalker):
            self.chains = walker.bind(metapath_list)
            if not 1 <= len(self.chains) <= 256:
                raise ValueError(f"{len(self.chains)} metapaths: the walk's key holds a metapath index in [0, 256)")
            self.metapaths = list(range(len(self.chains)))
        else:
            self.metapaths = [metapath_index(m) for m in metapath_list]
            self.chains = [None] * len(self.metapaths)
        self.counter = 0
        self.status: Optional[Tensor] = None       # sticky device word of the fixed path (1: a batch held duplicate seeds)

    def sample_blocks_fixed(self, seeds, counter=None, counter_add: int = 0):
        """``(seeds, [FixedBlock per metapath])``: :meth:`sample_blocks`'s blocks at the capacity ``B * (k + 1)`` (see
        :class:`FixedBlock`), with NO host read-back and shapes that depend on ``(B, k)`` alone, so the call can be captured in a
        hipGraph.  ``counter``: None (the sampler's next step counter), an int, or a 1-element uint64 / int64 device tensor the walk
        kernels read (effective counter ``counter + counter_add``).  Duplicate seeds: a host list / CPU tensor is checked here; for
        a device tensor the flag goes into the sampler's sticky device status word and :meth:`check` raises.  ``ValueError`` for an
        empty batch; the library's "exceeds the built maximum" error beyond ``ops.han_fixed_max_slab()`` slots."""
        w, k = self.walker, self.num_neighbors
        B = int(seeds.numel()) if torch.is_tensor(seeds) else int(np.asarray(seeds).size)
        if B == 0:
            raise ValueError("sample_blocks_fixed: an empty batch (B == 0) has no fixed-capacity block")
        ops.han_fixed_check(B, k)
        if torch.is_tensor(counter) and not counter.is_cuda:
            raise ValueError("sample_blocks_fixed: a counter tensor must live on the device; pass an int for a host counter")
        s32 = _seeds_on_device(w, seeds, check_dups=True)
        if counter is None:
            counter = self.counter
            self.counter += 1
        if self.status is None:
            self.status = torch.zeros(1, dtype=torch.int32, device=w.device)
        sorted_seeds, order = torch.sort(s32)
        blocks = []
        for mp, rels in zip(self.metapaths, self.chains):
            ends = _walk(w, mp, rels, s32, k, self.seed, counter, counter_add)
            rows, extra, counts = ops.han_block_rows(ends, s32, sorted_seeds)
            flat = torch.sort(extra.view(-1)).values
            rowptr, uniq, sizes = ops.han_block_relabel(counts, flat, sorted_seeds, k, self.status)
            col, dst, key, src_ids = ops.han_block_compact_fixed(rows, counts, rowptr, s32, sorted_seeds, order, uniq, sizes)
            # source-major orientation: a stable sort of the slots by their key (the local source id; the capacity for padding)
            keys_sorted, perm = torch.sort(key, stable=True)
            rowptrT, colT, slotT = ops.han_block_transpose(keys_sorted, perm, dst, B, k)
            blocks.append(FixedBlock(B, k, src_ids, rowptr, col, dst, rowptrT, colT, slotT, sizes))
        return seeds, blocks

    def check(self) -> None:
        """Reads the fixed path's sticky status word (ONE read-back) and raises the ``ValueError`` of :meth:`sample_blocks` if any
        batch of device seeds since the last call held duplicates; the word is cleared."""
        if self.status is not None and int(self.status.item()):
            self.status.zero_()
            raise ValueError("duplicate seeds: a block's target nodes are distinct (dgl.to_block raises too)")

    def sample_blocks(self, seeds, counter: Optional[int] = None):
        """``(seeds, [Block per metapath])``.  One host read-back per call (every block's edge and node counts, together)."""
        w = self.walker
        s32 = _seeds_on_device(w, seeds, check_dups=True)
        if counter is None:
            counter = self.counter
            self.counter += 1
        B, k, dev = s32.numel(), self.num_neighbors, w.device
        sorted_seeds, order = torch.sort(s32)
        seed_perm = order.to(torch.int32)
        dup = (sorted_seeds[1:] == sorted_seeds[:-1]).any().to(torch.int64).view(1) if B > 1 else torch.zeros(1, dtype=torch.int64, device=dev)
        slab = B * (k + 1)
        staged, sizes = [], [dup]
        for mp, rels in zip(self.metapaths, self.chains):
            ends = _walk(w, mp, rels, s32, k, self.seed, counter)
            rows, extra, counts = ops.han_block_rows(ends, s32, sorted_seeds)
            rowptr = torch.zeros(B + 1, dtype=torch.int32, device=dev)
            rowptr[1:] = torch.cumsum(counts, 0)
            # the distinct non-seed nodes, ascending: one sort of the slab, first occurrences scattered to their rank (slot `slab` of
            # the buffer collects everything else)
            flat = torch.sort(extra.view(-1)).values
            first = flat < INT32_MAX
            first[1:] &= flat[1:] != flat[:-1]
            rank = torch.cumsum(first, 0)
            uniq = torch.empty(slab + 1, dtype=torch.int32, device=dev)
            uniq[torch.where(first, rank - 1, slab)] = flat
            staged.append((rows, counts, rowptr, uniq))
            sizes += [rowptr[-1:].long(), rank[-1:] if slab else torch.zeros(1, dtype=torch.int64, device=dev)]
        host = torch.cat(sizes).tolist()                                # the one read-back
        if host[0]:
            raise ValueError("duplicate seeds: a block's target nodes are distinct (dgl.to_block raises too)")
        blocks = []
        seeds64 = s32.long()
        for i, (rows, counts, rowptr, uniq) in enumerate(staged):
            nnz, n_extra = int(host[1 + 2 * i]), int(host[2 + 2 * i])
            col, dst = ops.han_block_compact(rows, counts, rowptr, sorted_seeds, seed_perm, uniq, n_extra, nnz)
            n_src = B + n_extra
            # source-major orientation: a stable sort of the slots by source id
            colT_src, slots = torch.sort(col, stable=True)
            rowptrT = torch.searchsorted(colT_src, torch.arange(n_src + 1, dtype=torch.int32, device=dev)).to(torch.int32)
            slotT = slots.to(torch.int32)
            colT = dst[slots]
            src_ids = torch.cat([seeds64, uniq[:n_extra].long()])
            blocks.append(Block(B, n_src, src_ids, col.long(), dst.long(), rowptr, col, torch.arange(nnz, dtype=torch.int32, device=dev),
                                rowptrT, colT, slotT))
        return seeds, blocks


def load_subtensors(blocks: Sequence[Block], features: Tensor) -> List[Tensor]:
    """The feature rows of every block's source nodes."""
    return [features[b.src_ids] for b in blocks]


# --------------------------------------------------------------------------------------------------
# model (reference DGL_HAN/train_sampling.py; GATConv: dgl 0.7.1 nn/pytorch/conv/gatconv.py on a block)
# --------------------------------------------------------------------------------------------------

class GATConv(nn.Module):
    """DGL 0.7.1 ``GATConv`` on a block, as mini-batch HAN uses it (``allow_zero_in_degree=True`` is accepted: every target of a
    sampled block has its self-loop): ``fs = fc(feat_drop(h_src))``, ``el`` from all ``n_src`` rows, ``er`` from the first ``n_dst``.
    ``state_dict`` keys and shapes are the full-batch ``han.GATConv``'s."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0., negative_slope=0.2, residual=False,
                 activation=None, allow_zero_in_degree=False, bias=True):
        super().__init__()
        if residual or not bias:
            raise ValueError("GATConv: residual / bias=False are not built (HAN uses neither)")
        if activation is not F.elu:
            raise ValueError("GATConv: the HIP hop is built with HAN's activation, F.elu")
        self._num_heads, self._in_feats, self._out_feats = num_heads, in_feats, out_feats
        self._allow_zero_in_degree = bool(allow_zero_in_degree)
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.attn_r = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop, self.attn_drop, self.negative_slope = float(feat_drop), float(attn_drop), float(negative_slope)
        self.bias = nn.Parameter(torch.empty(num_heads * out_feats))
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain('relu')
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        nn.init.constant_(self.bias, 0)

    def forward(self, block: Block, feat: Tensor, out: Optional[Tensor] = None, col_block: int = 0) -> Tensor:
        """[n_dst, H, C] -- or, with ``out``, the stacked buffer itself with column block ``col_block`` filled."""
        H, C = self._num_heads, self._out_feats
        if feat.shape[0] != block.n_src:
            raise ValueError(f"GATConv: {feat.shape[0]} feature rows for a block of {block.n_src} source nodes")
        h = dense.hash_dropout(feat, self.feat_drop, self.training)
        fs = dense.linear(h, self.fc.weight, None)
        f3 = fs.view(-1, H, C)
        el = (f3 * self.attn_l).sum(-1)
        er = (f3[:block.n_dst] * self.attn_r).sum(-1)
        y = han_block_propagate(fs, el, er, block, H, self.negative_slope, self.bias, self.attn_drop if self.training else 0.0, out,
                                col_block)
        return y if out is not None else y.view(-1, H, C)


class HANLayer(nn.Module):
    def __init__(self, num_metapath, in_size, out_size, layer_num_heads, dropout):
        super().__init__()
        self.gat_layers = nn.ModuleList()
        for _ in range(num_metapath):
            self.gat_layers.append(GATConv(in_size, out_size, layer_num_heads, dropout, dropout, activation=F.elu,
                                           allow_zero_in_degree=True))
        self.semantic_attention = SemanticAttention(in_size=out_size * layer_num_heads)
        self.num_metapath = num_metapath

    def forward(self, block_list, h_list) -> Tensor:
        M = len(block_list)
        if M != len(h_list) or M > len(self.gat_layers):
            raise ValueError(f"HANLayer: {M} blocks, {len(h_list)} feature tensors, {len(self.gat_layers)} metapaths")
        n_dst = block_list[0].n_dst
        if any(b.n_dst != n_dst for b in block_list):
            raise ValueError("HANLayer: the blocks of one batch share their target nodes")
        d = self.gat_layers[0]._num_heads * self.gat_layers[0]._out_feats
        z = torch.empty((n_dst, M * d), dtype=torch.float32, device=h_list[0].device)   # the reference's torch.stack(..., dim=1)
        for i, blk in enumerate(block_list):
            z = self.gat_layers[i](blk, h_list[i], out=z, col_block=i)
        return self.semantic_attention(z.view(n_dst, M, d))


class HAN(nn.Module):
    def __init__(self, num_metapath, in_size, hidden_size, out_size, num_heads, dropout):
        super().__init__()
        self.layers = nn.ModuleList()
        self.layers.append(HANLayer(num_metapath, in_size, hidden_size, num_heads[0], dropout))
        for l in range(1, len(num_heads)):
            self.layers.append(HANLayer(num_metapath, hidden_size * num_heads[l - 1], hidden_size, num_heads[l], dropout))
        self.predict = nn.Linear(hidden_size * num_heads[-1], out_size)

    def forward(self, g, h) -> Tensor:
        if len(self.layers) != 1:
            raise ValueError("mini-batch HAN is single-layer: the reference hands the same blocks (and the blocks' input features) to "
                             f"every layer, which cannot work for len(num_heads) = {len(self.layers)} > 1")
        h = self.layers[0](g, h)
        return dense.linear(h, self.predict.weight, self.predict.bias)


# --------------------------------------------------------------------------------------------------
# the whole step as one hipGraph
# --------------------------------------------------------------------------------------------------

class GraphedSampledStep:
    """One mini-batch training step -- the device walk counter += 1, ``sample_blocks_fixed`` from a static int32 seed buffer, the
    feature gather, forward, loss against a static label buffer, backward, optimizer -- captured as ONE graph on one stream
    (``graphs.GraphedTrainStep``'s protocol: warm-up on the capture stream, ``dense.device_seed_counter`` for the dropout masks,
    ``dense.deferred_param_grads``, a capturable optimizer, ``restore=True`` puts parameters and optimizer state back so that the
    first replay is step 1).  ``loss = step(ids)`` copies ``ids`` and ``labels[ids]`` into the static buffers, replays and returns
    the static loss tensor.  The batch size is fixed here; a shorter last batch goes through the eager path.  Replay ``i`` walks
    with the step counter the sampler's next eager call would have used, and the sampler's counter advances with it."""

    def __init__(self, model: nn.Module, sampler: HANSampler, features: Tensor, labels: Tensor, loss_fn, optimizer, batch_size: int,
                 warmup: int = 3, train_mode: bool = True, restore: bool = True):
        from .graphs import _side_stream_warmup
        from .optim import FusedAdam
        for grp in optimizer.param_groups:
            if not grp.get("capturable", False):
                raise _lib.AllSetHipError("GraphedSampledStep needs a capturable optimizer (optim.FusedAdam, or "
                                          "torch.optim.Adam(..., capturable=True))")
        B = int(batch_size)
        if B < 1:
            raise ValueError("GraphedSampledStep: batch_size must be >= 1")
        ops.han_fixed_check(B, sampler.num_neighbors)
        _lib.require_device(features, labels)
        if B > sampler.walker.n:
            raise ValueError(f"GraphedSampledStep: batch_size {B} exceeds the {sampler.walker.n} nodes seeds are drawn from")
        dev = features.device
        self.model, self.sampler, self.optimizer, self.labels, self.batch_size = model, sampler, optimizer, labels, B
        self.ids = torch.arange(B, dtype=torch.int32, device=dev)                 # warm-up seeds: distinct and in range
        self.batch_labels = labels[:B].clone()
        self.walk_counter = torch.zeros(1, dtype=torch.int64, device=dev)
        self.counter = torch.zeros(1, dtype=torch.int64, device=dev)             # the dropout masks' device seed counter
        # (derived from the sampler's seed, not drawn: building the step leaves torch's generators where the eager driver has them)
        self.counter.fill_(((sampler.seed + 1) * 0x9E3779B97F4A7C15) & 0x3FFFFFFFFFFFFFFF)
        model.train(train_mode)
        one = self._one = torch.ones((), dtype=torch.float32, device=dev)
        fused = isinstance(optimizer, FusedAdam)

        def one_step():
            optimizer.zero_grad(set_to_none=True)
            self.walk_counter.add_(1)
            _, blocks = sampler.sample_blocks_fixed(self.ids, counter=self.walk_counter)
            loss = loss_fn(model(blocks, load_subtensors(blocks, features)), self.batch_labels)
            with dense.deferred_param_grads(bump_i64=self.counter, bump_f32=optimizer.step_counters if fused else None):
                loss.backward(one if (loss.dim() == 0 and loss.dtype == one.dtype) else None)
            if fused:
                optimizer.step(counters_advanced=True)
            else:
                optimizer.step()
            return loss

        params = [p for grp in optimizer.param_groups for p in grp["params"]]
        if restore:
            with torch.no_grad():
                p_snap = [p.detach().clone() for p in params]
                s_snap = {p: {k: v.clone() for k, v in optimizer.state.get(p, {}).items() if torch.is_tensor(v)} for p in params}
                b_snap = [(b, b.detach().clone()) for b in model.buffers()]
        with torch.cuda.device(dev), dense.device_seed_counter(self.counter):
            st = _side_stream_warmup(one_step, max(1, warmup))
            self.graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.graph, stream=st):
                self.loss = one_step()
        if restore:
            with torch.no_grad():
                for p, snap in zip(params, p_snap):
                    p.copy_(snap)
                    for k, v in optimizer.state.get(p, {}).items():
                        if torch.is_tensor(v):
                            v.copy_(s_snap[p][k]) if k in s_snap[p] else v.zero_()
                for b, snap in b_snap:
                    b.copy_(snap)
        self._walk_mirror: Optional[int] = None                                   # the device walk counter's value, as the host knows it

    def step(self, ids: Tensor) -> Tensor:
        if ids.numel() != self.batch_size:
            raise ValueError(f"GraphedSampledStep: {ids.numel()} seeds for a step captured at batch size {self.batch_size}; run a "
                             "shorter batch through the eager path")
        _lib.require_device(ids)
        self.ids.copy_(ids.view(-1))
        torch.index_select(self.labels, 0, ids.view(-1).long(), out=self.batch_labels)
        want = self.sampler.counter - 1                                          # the graph adds one before it walks
        if self._walk_mirror != want:
            self.walk_counter.fill_(want)
        self.graph.replay()
        self._walk_mirror = want + 1
        self.sampler.counter += 1
        return self.loss

    __call__ = step


# --------------------------------------------------------------------------------------------------
# driver (reference DGL_HAN/train_sampling.py)
# --------------------------------------------------------------------------------------------------

def _batches(ids: Tensor, batch_size: int):
    return [ids[i:i + batch_size] for i in range(0, ids.numel(), batch_size)]


def evaluate(model, g, metapath_list, num_neighbors, features, labels, val_nid, loss_fcn, batch_size, seed: int = 0, counter: int = 0):
    """The reference's ``evaluate``: ``2 * num_neighbors`` walks, batches in order, the predictions of all batches concatenated for
    the scores -- and the loss of the LAST batch alone returned (the reference's quirk; ``EarlyStopping`` consumes it)."""
    model.eval()
    sampler = HANSampler(g, metapath_list, num_neighbors=num_neighbors * 2, seed=seed)
    logits_all, labels_all = [], []
    loss = None
    with torch.no_grad():
        for step, ids in enumerate(_batches(val_nid, batch_size)):
            seeds, blocks = sampler.sample_blocks(ids, counter=counter + step)
            logits = model(blocks, load_subtensors(blocks, features))
            batch_labels = labels[ids]
            loss = loss_fcn(logits, batch_labels)
            logits_all.append(logits)
            labels_all.append(batch_labels)
    if loss is None:
        raise ValueError("evaluate: no nodes to evaluate on")
    return (loss,) + score(torch.cat(logits_all), torch.cat(labels_all))


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser('mini-batch HAN')
    p.add_argument('-s', '--seed', type=int, default=1, help='Random seed')
    p.add_argument('--hetero', action='store_true', help="one typed graph and metapaths of edge types (the reference's ACMRaw branch; "
                   "--dataset synthetic) instead of the hypergraph's VEV / EVE walks")
    p.add_argument('--batch_size', type=int, default=32)
    p.add_argument('--num_neighbors', type=int, default=20)
    p.add_argument('--lr', type=float, default=0.001)
    p.add_argument('--hidden_units', type=int, default=8)
    p.add_argument('--dropout', type=float, default=0.6)
    p.add_argument('--weight_decay', type=float, default=0.001)
    p.add_argument('--num_epochs', type=int, default=100)
    p.add_argument('--patience', type=int, default=10)
    p.add_argument('--dataset', type=str, default='synthetic', help="'synthetic' or a dataset name train.py loads (with "
                   "--raw_data_dir / --processed_data)")
    p.add_argument('--runs', type=int, default=20)
    p.add_argument('--cuda', type=int, default=0)
    p.add_argument('--train_prop', type=float, default=0.5)
    p.add_argument('--valid_prop', type=float, default=0.25)
    p.add_argument('--feature_noise', type=float, default=1)
    # additions of this driver: where train.py's loaders find a named dataset
    p.add_argument('--raw_data_dir', default=None)
    p.add_argument('--processed_data', default=None)
    p.add_argument('--fixed_blocks', action='store_true', help='train over fixed-capacity blocks built without a host read-back '
                   '(HANSampler.sample_blocks_fixed) and optim.FusedAdam')
    p.add_argument('--graph_step', action='store_true', help='implies --fixed_blocks: full batches replay one captured hipGraph '
                   '(GraphedSampledStep); the last, shorter batch of an epoch and evaluation run eagerly')
    return p


def setup(args: dict) -> dict:
    args['num_heads'] = [8]
    args['fixed_blocks'] = bool(args.get('fixed_blocks') or args.get('graph_step'))       # --graph_step implies --fixed_blocks
    np.random.seed(args['seed'])
    torch.manual_seed(args['seed'])
    args['device'] = f"cuda:{args['cuda']}"
    return args


def load_data(args: dict):
    """``(walker, features, labels, num_classes)`` on ``args['device']``; with ``--hetero`` the walker is over the typed graph of
    ``han_hetero.load_data`` and the labelled nodes are its papers."""
    if args.get('hetero'):
        g, features, labels, num_classes = han_hetero.load_data(args)
        return TypedMetapathWalker(g), features, labels, num_classes
    from . import train
    from .preprocessing import ExtractV2E
    targs = SimpleNamespace(dname=args['dataset'], raw_data_dir=args.get('raw_data_dir'), processed_data=args.get('processed_data'),
                            feature_noise=str(args['feature_noise']), seed=args['seed'])
    data = ExtractV2E(train.load_data(targs))
    data = data.to(args['device'])
    features, labels = node_features(data)
    return MetapathWalker(data, e_base=_first(data.n_x)), features, labels, int(targs.num_classes)


def main(args: dict) -> dict:
    walker, features, labels, num_classes = load_data(args)
    metapath_list = META_PATHS if args.get('hetero') else DEFAULT_METAPATHS
    k, bs = args['num_neighbors'], args['batch_size']
    if 2 * k > ops.HAN_MAX_WALKS:
        raise ValueError(f"--num_neighbors {k}: evaluation samples twice as many walks and the kernel is built for {ops.HAN_MAX_WALKS}")
    history = {'acc': [], 'micro_f1': [], 'macro_f1': [], 'time': [], 'train_loss': []}
    shuffle = torch.Generator().manual_seed(args['seed'])
    for run in range(args['runs']):
        split = rand_train_test_idx(labels, args['train_prop'], args['valid_prop'])
        train_nid, val_nid, test_nid = split['train'], split['valid'], split['test']
        sample_seed = args['seed'] * 1000003 + run
        sampler = HANSampler(walker, metapath_list, k, seed=sample_seed)
        model = HAN(num_metapath=len(metapath_list), in_size=features.shape[1], hidden_size=args['hidden_units'], out_size=num_classes,
                    num_heads=args['num_heads'], dropout=args['dropout']).to(args['device'])
        stopper = EarlyStopping(patience=args['patience'])
        loss_fn = torch.nn.CrossEntropyLoss()
        fixed = bool(args.get('fixed_blocks') or args.get('graph_step'))
        graphed = None
        if fixed:
            from .optim import FusedAdam
            optimizer = FusedAdam(model.parameters(), lr=args['lr'], weight_decay=args['weight_decay'])
            if args.get('graph_step') and train_nid.numel() >= bs:
                graphed = GraphedSampledStep(model, sampler, features, labels, loss_fn, optimizer, bs)
        else:
            optimizer = torch.optim.Adam(model.parameters(), lr=args['lr'], weight_decay=args['weight_decay'])
        start = time.time()
        epoch_losses = []
        eval_counter = 1 << 40                                         # evaluation draws from its own range of step counters
        for epoch in range(args['num_epochs']):
            model.train()
            perm = torch.randperm(train_nid.numel(), generator=shuffle).to(train_nid.device)       # DataLoader(shuffle=True)
            losses = []
            for ids in _batches(train_nid[perm], bs):
                if graphed is not None and ids.numel() == bs:
                    losses.append(graphed.step(ids).detach().clone())
                    continue
                seeds, blocks = sampler.sample_blocks_fixed(ids) if fixed else sampler.sample_blocks(ids)
                logits = model(blocks, load_subtensors(blocks, features))
                loss = loss_fn(logits, labels[ids])
                optimizer.zero_grad()
                loss.backward()
                optimizer.step()
                losses.append(loss.detach())
            epoch_losses.append(float(torch.stack(losses).mean()))
            if fixed:
                sampler.check()                                            # the epoch's one read of the duplicate-seed status word
            val_loss, val_acc, _, _ = evaluate(model, walker, metapath_list, k, features, labels, val_nid, loss_fn, bs, sample_seed,
                                               eval_counter)
            eval_counter += 1 << 20
            if stopper.step(float(val_loss), val_acc, model):
                break
        stopper.load_checkpoint(model)
        _, test_acc, test_micro, test_macro = evaluate(model, walker, metapath_list, k, features, labels, test_nid, loss_fn, bs,
                                                       sample_seed, eval_counter)
        history['acc'].append(100 * test_acc)
        history['micro_f1'].append(100 * test_micro)
        history['macro_f1'].append(100 * test_macro)
        history['train_loss'].append(epoch_losses)
        history['time'].append(time.time() - start)
    print(f">> Final test acc: {np.mean(history['acc']):.2f}, std: {np.std(history['acc']):.2f}; "
          f"test marco f1: {np.mean(history['macro_f1']):.2f}, std: {np.std(history['macro_f1']):.2f}")
    print(f">> Train time per run: {np.mean(history['time']):.2f}, std: {np.std(history['time']):.2f}")
    return history


if __name__ == '__main__':
    main(setup(build_parser().parse_args().__dict__))
