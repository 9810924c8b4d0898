"""AllSet's edge-list preprocessing (the step immediately before the hot path) as vectorised
tensor programs that run wherever the ids live (ROCm device or host).

Same function names, ``data`` attributes and results as reference ``src/preprocessing.py``:

* ``ExtractV2E``        (:394-409)  [V|E ; E|V] block edge list -> the V->E half, sorted by vertex id
* ``Add_Self_Loops``    (:412-448)  one new singleton hyperedge per vertex that is not already alone in one
* ``norm_contruction``  (:451-469)  per-incidence ``norm``: 'all_one' (int64 ones) or 'deg_half_sym'
* ``expand_edge_index`` (:22-144)   "exclude-self" expansion: hyperedge e of size k becomes k hyperedges e_i,
                                     e_i containing every member except the i-th
* ``ConstructH_pairs``  (:186-203)  ``ConstructH`` as sorted, de-duplicated (vertex, hyperedge) pairs instead of a dense matrix,
                                     and ``generate_norm_UniGNN`` (train.py:405-412): UniGCNII's degree scales

The reference implements these with Python loops over vertices / hyperedges and ``i not in list`` scans --
O(n_V * k), minutes at 1M vertices.  Here each is a handful of sorts / bincounts / prefix sums.  Where the
reference's result depends on an unstable sort (``torch.sort`` / ``argsort`` ties, :398,446,141) the order within
equal vertex ids is unspecified there; these versions use stable sorts, i.e. they return one of the orders the
reference may return (tests compare per-vertex multisets).
"""
from __future__ import annotations

from typing import Optional

import torch

Tensor = torch.Tensor


def _first(v) -> int:
    """``data.n_x[0]`` / ``data.num_hyperedges[0]`` may be tensors, arrays, lists or plain ints."""
    try:
        v = v[0]
    except (TypeError, IndexError):
        pass
    return int(v)


def _sort_by_vertex(edge_index: Tensor) -> Tensor:
    order = torch.argsort(edge_index[0], stable=True)
    return edge_index[:, order].to(torch.int64)


def ExtractV2E(data):
    """Keep the vertex->hyperedge half of a ``[V|E ; E|V]`` edge list (reference preprocessing.py:394-409)."""
    edge_index = _sort_by_vertex(data.edge_index)
    num_nodes = _first(data.n_x)
    num_hyperedges = _first(data.num_hyperedges)
    if not ((num_nodes + num_hyperedges - 1) == int(data.edge_index[0].max())):
        print('num_hyperedges does not match! 1')
        return
    # sorted by row 0: the V->E half is the prefix whose source id is a vertex id
    cidx = int(torch.searchsorted(edge_index[0].contiguous(), torch.tensor(num_nodes, device=edge_index.device)))
    data.edge_index = edge_index[:, :cidx].contiguous()
    return data


def Add_Self_Loops(data):
    """Append a new singleton hyperedge for every vertex that is not already the only member of some hyperedge
    (reference preprocessing.py:412-448).  New ids continue after the largest hyperedge id, in increasing vertex
    order; ``data.totedges`` is set as in the reference."""
    edge_index = data.edge_index
    num_nodes = _first(data.n_x)
    num_hyperedges = _first(data.num_hyperedges)
    if not ((num_nodes + num_hyperedges - 1) == int(edge_index[1].max())):
        print('num_hyperedges does not match! 2')
        return
    dev = edge_index.device
    e_min = int(edge_index[1].min())
    sizes = torch.bincount(edge_index[1] - e_min)
    alone = sizes[edge_index[1] - e_min] == 1                       # incidences of size-1 hyperedges
    skip = torch.zeros(num_nodes, dtype=torch.bool, device=dev)
    skip[edge_index[0][alone]] = True
    new_v = (~skip).nonzero().reshape(-1)
    new_e = int(edge_index[1].max()) + 1 + torch.arange(new_v.numel(), device=dev, dtype=torch.int64)
    n_skipped = int(alone.sum())                                    # the reference counts list entries (:440)
    data.totedges = num_hyperedges + num_nodes - n_skipped
    edge_index = torch.cat([edge_index, torch.stack([new_v, new_e])], dim=1)
    data.edge_index = _sort_by_vertex(edge_index).contiguous()
    return data


def norm_contruction(data, option='all_one', TYPE='V2E'):
    """Per-incidence weights (reference preprocessing.py:451-469; the reference's spelling is kept).
    'all_one': int64 ones (the default train.py uses).  'deg_half_sym': D_v^-1/2 * D_e^-1/2."""
    if TYPE == 'V2E':
        if option == 'all_one':
            data.norm = torch.ones_like(data.edge_index[0])
        elif option == 'deg_half_sym':
            v, e = data.edge_index[0], data.edge_index[1]
            cidx = e.min()
            Vdeg = torch.bincount(v).to(torch.float32)
            HEdeg = torch.bincount(e - cidx).to(torch.float32)
            data.norm = Vdeg.pow(-0.5)[v] * HEdeg.pow(-0.5)[e - cidx]
    elif TYPE == 'V2V':
        data.edge_index, data.norm = gcn_norm(data.edge_index, data.norm, add_self_loops=True)
    return data


# ---- clique expansion of the CEGCN baseline (reference preprocessing.py:343-391, 466-468; csrc/clique.hip) ------------------------
# Device programs: ids on the host go through the current ROCm device and come back to the host, so train.py's order
# (preprocess, then move ``data`` to the device) is kept.

def _on_device(t: Tensor) -> Tensor:
    if t.is_cuda:
        return t
    if not torch.cuda.is_available():
        from ._lib import AllSetHipError
        raise AllSetHipError("the clique expansion runs on a ROCm device (csrc/clique.hip); no device is available")
    return t.to(torch.device('cuda', torch.cuda.current_device()))


def ConstructV2V(data):
    """Clique expansion of a V->E edge list (reference preprocessing.py:343-391): every pair ``(i, j)``, ``i < j``, of members of a
    hyperedge with at least two members, in ONE direction (``edge_index[0] = i``), once; ``data.norm`` = the number of hyperedges
    sharing the pair (float32).  Size-1 hyperedges contribute nothing.  The reference emits pairs in dict insertion order; here
    they come sorted by ``(i, j)``.  Duplicate incidences (which the loaders never produce) count once."""
    ei = data.edge_index
    home = ei.device
    ei = _on_device(ei)
    dev = ei.device
    v, e = ei[0], ei[1]
    if v.numel() == 0:
        data.edge_index = torch.zeros((2, 0), dtype=torch.int64, device=home)
        data.norm = torch.zeros(0, dtype=torch.float32, device=home)
        return data
    e = e - e.min()
    n_v = int(v.max()) + 1
    key = torch.unique(e * n_v + v)                              # sorted by (hyperedge, vertex): members ascending
    e, v = key // n_v, key % n_v
    n_e = int(e[-1]) + 1
    rowptr = torch.zeros(n_e + 1, dtype=torch.int32, device=dev)
    rowptr[1:] = torch.cumsum(torch.bincount(e, minlength=n_e), 0).to(torch.int32)
    from . import ops
    pairs = ops.clique_pairs(rowptr, v.to(torch.int32), e.to(torch.int32))
    pairs, mult = torch.unique_consecutive(torch.sort(pairs).values, return_counts=True)
    data.edge_index = torch.stack([pairs >> 32, pairs & 0xFFFFFFFF]).to(home)
    data.norm = mult.to(torch.float32).to(home)
    return data


def _dedup_by_hyperedge(edge_index: Tensor):
    """``(e, v)`` of the distinct (vertex, hyperedge) pairs sorted by (hyperedge, vertex), hyperedge ids re-based to 0 -- the rows
    ``ConstructV2V`` expands."""
    v, e = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    e = e - e.min()
    n_v = int(v.max()) + 1
    key = torch.unique(e * n_v + v)
    return key // n_v, key % n_v


def clique_implicit_structure(edge_index: Tensor, n: Optional[int] = None) -> dict:
    """What the GCN hop over the clique expansion of the V->E list ``edge_index`` needs, WITHOUT the expansion (pure torch, any device;
    all int64 unless noted).  With the distinct members of each hyperedge in ascending vertex order, one position per incidence:

    ``e_rowptr`` [n_e + 1], ``member`` [nnz]: the hyperedge-major CSR (``member[p]`` = the vertex at position p);
    ``rank`` [nnz]: the number of smaller members of p's hyperedge -- the pairs (i, member[p]), i < member[p], p's hyperedge emits;
    ``v_rowptr`` [n + 1], ``v_pos`` [nnz]: the vertex-major CSR whose columns are positions of the first;
    ``N``: (the largest vertex in a hyperedge of two or more) + 1 -- the ``edge_index.max() + 1`` of ``gcn_norm`` over the pairs;
    ``loop`` bool [n]: ``j < N``, the vertices ``gcn_norm`` gives a self-loop;
    ``deg`` [n]: ``loop[j] + sum of rank over j's positions`` -- the integer in-degree (with multiplicities) ``gcn_norm`` sums.

    ``n`` (default: largest vertex id + 1) is the number of vertex rows.  Raises ``ValueError`` when no hyperedge has two members
    (the expansion is empty, which ``gcn_norm`` refuses)."""
    if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.shape[1] == 0:
        raise ValueError(f"gcn_norm: expected a non-empty [2, E] edge list, got an expansion of {tuple(edge_index.shape)} incidences "
                         "without a pair")
    if int(edge_index[0].min()) < 0:
        raise ValueError("gcn_norm: negative vertex id")
    e, v = _dedup_by_hyperedge(edge_index)
    dev = v.device
    n_e = int(e[-1]) + 1
    n = int(v.max()) + 1 if n is None else int(n)
    if int(v.max()) >= n:
        raise ValueError(f"clique_implicit_structure: vertex ids reach {int(v.max())} but there are {n} vertex rows")
    size = torch.bincount(e, minlength=n_e)
    e_rowptr = torch.zeros(n_e + 1, dtype=torch.int64, device=dev)
    e_rowptr[1:] = torch.cumsum(size, 0)
    paired = size[e] >= 2
    if not bool(paired.any()):
        raise ValueError("gcn_norm: expected a non-empty [2, E] edge list, got (2, 0): no hyperedge has two members")
    rank = torch.arange(v.numel(), device=dev) - e_rowptr[e]
    N = int(v[paired].max()) + 1
    loop = torch.arange(n, device=dev) < N
    deg = torch.zeros(n, dtype=torch.int64, device=dev).index_add_(0, v, rank) + loop.to(torch.int64)
    v_pos = torch.argsort(v, stable=True)
    v_rowptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    v_rowptr[1:] = torch.cumsum(torch.bincount(v, minlength=n), 0)
    return dict(e_rowptr=e_rowptr, member=v, rank=rank, v_rowptr=v_rowptr, v_pos=v_pos, N=N, loop=loop, deg=deg, n=n, n_e=n_e)


def ConstructV2V_implicit(data):
    """CEGCN's preprocessing WITHOUT the clique expansion: where ``ConstructV2V`` + ``norm_contruction(TYPE=
    'V2V')`` write one weighted edge per vertex pair, this keeps the V->E list -- ``data.edge_index`` = the distinct (vertex, hyperedge)
    pairs (duplicates count once, as in ``ConstructV2V``; hyperedge ids as given), sorted by vertex -- and the GCN hop is computed from
    prefix sums over it (``baselines.ImplicitCEGraph``, ``functional.clique_propagate``).  Sets ``data.norm = None``,
    ``data.clique_expansion = True`` and ``data.clique_implicit = True``.  Pure torch, on the device the ids live on.  Raises the
    ``ValueError`` of ``gcn_norm`` when no hyperedge has two members."""
    ei = data.edge_index
    if ei.dim() != 2 or ei.shape[0] != 2 or ei.shape[1] == 0:
        raise ValueError(f"gcn_norm: expected a non-empty [2, E] edge list, got an expansion of {tuple(ei.shape)} incidences without a pair")
    e_min = ei[1].min()
    e, v = _dedup_by_hyperedge(ei)
    if int(torch.bincount(e).max()) < 2:
        raise ValueError("gcn_norm: expected a non-empty [2, E] edge list, got (2, 0): no hyperedge has two members")
    data.edge_index = _sort_by_vertex(torch.stack([v, e + e_min])).contiguous()
    data.norm = None
    data.clique_expansion = True
    data.clique_implicit = True
    return data


def gcn_norm(edge_index, edge_weight=None, add_self_loops=True):
    """torch_geometric 1.6.3 ``gcn_norm(edge_index, edge_weight, add_self_loops=True)`` as ``norm_contruction(TYPE='V2V')`` calls it:
    ``N = edge_index.max() + 1`` (not the vertex count: ids >= N get no loop), one self-loop of weight 1 per id < N,
    ``deg[j]`` = the weights into ``j``, ``w = deg^-1/2[src] * m * deg^-1/2[dst]``.  Returns ``(edge_index [pairs | loops], w)``
    on the device ``edge_index`` came from.  The graph must have no self-loops (``ConstructV2V`` emits none).  The degree is a
    float atomic sum: exact and run-to-run identical for integer weights below 2^24 (``ConstructV2V``'s multiplicities); other
    weights may differ from run to run in their last bits."""
    if not add_self_loops:
        raise NotImplementedError("gcn_norm(add_self_loops=False) is not built (the reference's V2V branch adds them)")
    home = edge_index.device
    ei = _on_device(edge_index)
    if ei.dim() != 2 or ei.shape[0] != 2 or ei.shape[1] == 0:
        raise ValueError(f"gcn_norm: expected a non-empty [2, E] edge list, got {tuple(ei.shape)}")
    src, dst = ei[0].to(torch.int64), ei[1].to(torch.int64)
    if bool((src == dst).any()):
        raise ValueError("gcn_norm: the edge list has self-loops; the clique expansion (ConstructV2V) never emits any")
    if int(ei.min()) < 0:
        raise ValueError("gcn_norm: negative vertex id")
    n = int(ei.max()) + 1
    m = edge_weight.to(device=ei.device, dtype=torch.float32) if edge_weight is not None else None
    if m is not None and m.numel() != src.numel():
        raise ValueError(f"gcn_norm: {m.numel()} weights for {src.numel()} edges")
    from . import ops
    out, w = ops.gcn_norm(src, dst, m, n)
    return out.to(home), w.to(home)


def expand_edge_index(data, edge_th=0):
    """"Exclude-self" expansion (reference preprocessing.py:22-144; ``--exclude_self`` in train.py).

    Hyperedge e = {n_1..n_k} (k > 1) becomes k hyperedges e_1..e_k with e_i = e minus n_i, i.e. node n_j is
    connected to every e_i with i != j; a size-1 hyperedge is kept as one hyperedge.  New hyperedge ids are
    consecutive from ``n_x`` in the order (original hyperedge id, member position); hyperedges larger than
    ``edge_th`` (> 0) are dropped without consuming ids.  Result sorted by node id."""
    edge_index = data.edge_index
    dev = edge_index.device
    num_nodes = _first(data.n_x)
    num_edges = int(data.totedges) if hasattr(data, 'totedges') else _first(data.num_hyperedges)
    v, e = edge_index[0], edge_index[1] - num_nodes
    valid = (e >= 0) & (e < num_edges)
    v, e = v[valid], e[valid]
    order = torch.argsort(e, stable=True)                            # members of a hyperedge in edge-list order
    v, e = v[order], e[order]
    sizes = torch.bincount(e, minlength=num_edges)
    keep_e = sizes > 0
    if edge_th > 0:
        keep_e &= sizes <= edge_th
    ids_used = torch.where(keep_e, sizes, torch.zeros_like(sizes))   # a kept hyperedge of size k consumes k ids
    base = num_nodes + torch.cumsum(ids_used, 0) - ids_used         # first new id of each original hyperedge
    start = torch.cumsum(sizes, 0) - sizes
    pos = torch.arange(e.numel(), device=dev) - start[e]             # member position j inside its hyperedge
    keep_inc = keep_e[e]
    v, e, pos = v[keep_inc], e[keep_inc], pos[keep_inc]
    k = sizes[e]
    # every (hyperedge, member j) emits k candidates i = 0..k-1; drop i == j unless the hyperedge is a singleton
    rep_v = v.repeat_interleave(k)
    rep_e = e.repeat_interleave(k)
    rep_j = pos.repeat_interleave(k)
    first = torch.cumsum(k, 0) - k
    i = torch.arange(rep_v.numel(), device=dev) - first.repeat_interleave(k)
    keep = (i != rep_j) | (sizes[rep_e] == 1)
    new_v = rep_v[keep]
    new_e = base[rep_e[keep]] + i[keep]
    data.edge_index = _sort_by_vertex(torch.stack([new_v, new_e])).contiguous()
    return data


EXCLUDE_SELF_NORMTYPES = ('all_one', 'deg_half_sym')


def exclude_self(data, normtype='all_one', attention=False):
    """The exclude-self mode WITHOUT the expansion: ``data.edge_index`` (the V->E list, hyperedge ids from ``n_x``) stays as it is and
    ``SetGNN`` (Deep Sets convs) computes what it would compute over ``expand_edge_index(data)`` with
    ``norm_contruction(option=normtype)`` from leave-one-out sums over the plain incidence (incidence.LeaveOneOutIncidence,
    csrc/loo.hip): O(nnz) incidences in memory and per pass instead of sum k (k - 1).  Sets ``data.exclude_self = True``,
    ``data.exclude_self_normtype`` and ``data.norm`` = int64 ones of the unexpanded length (the normalisation of the expanded list is
    applied inside the aggregation).  ``attention=True`` (sets ``data.exclude_self_attention``) lets the PMA convs of AllSetTransformer take
    the data too -- a leave-one-out softmax (csrc/loo_softmax.hip; PMA ignores ``norm``, so ``normtype`` plays no part there);
    without it a PMA conv refuses unexpanded data.  Refuses what the expansion would silently drop or what is ill-defined under it: hyperedge ids
    outside ``[n_x, n_x + number of hyperedges)`` and repeated (vertex, hyperedge) pairs."""
    if normtype not in EXCLUDE_SELF_NORMTYPES:
        raise ValueError(f"exclude_self: normtype {normtype!r} is not built without the expansion ({' | '.join(EXCLUDE_SELF_NORMTYPES)})")
    ei = data.edge_index
    if ei.dim() != 2 or ei.shape[0] != 2 or ei.dtype != torch.int64:
        raise ValueError(f"exclude_self: edge_index must be int64 [2, nnz], got {ei.dtype} {tuple(ei.shape)}")
    num_nodes = _first(data.n_x)
    num_edges = int(data.totedges) if hasattr(data, 'totedges') else _first(data.num_hyperedges)
    if ei.shape[1] > 0:
        v, e = ei[0], ei[1] - num_nodes
        if int(v.min()) < 0 or int(v.max()) >= num_nodes:
            raise ValueError(f"exclude_self: vertex ids span [{int(v.min())}, {int(v.max())}] but n_x = {num_nodes}")
        if int(e.min()) < 0 or int(e.max()) >= num_edges:
            raise ValueError(f"exclude_self: hyperedge ids span [{int(ei[1].min())}, {int(ei[1].max())}], outside "
                             f"[{num_nodes}, {num_nodes + num_edges}) (expand_edge_index would drop them)")
        if int(torch.unique(e * num_nodes + v).numel()) != ei.shape[1]:
            raise ValueError("exclude_self: duplicate (vertex, hyperedge) incidences (coalesce the edge list first)")
    data.exclude_self = True
    data.exclude_self_normtype = normtype
    data.exclude_self_attention = bool(attention)
    data.norm = torch.ones_like(ei[0])
    return data


# ---- degree scales of the hypergraph-convolution baselines (HCHA / HGNN / HNHN) ---------------------------------------------------
# Computed once, on the device the ids live on, from the [V; E] edge list (no dense incidence matrix); stored as attributes of
# ``data``.  A reciprocal of zero is 0 (the reference's ``D[D == inf] = 0``); a power of zero with a negative exponent is inf, as in
# the reference's numpy ``DV ** beta``.

def _vertex_edge_ids(edge_index: Tensor, num_nodes: int):
    v, e = edge_index[0], edge_index[1]
    e = e - e.min() if e.numel() else e
    num_edges = int(e.max()) + 1 if e.numel() else 0          # the reference's max(id) + 1 (layers.py:422-423)
    return v, e, num_nodes, num_edges


def _inv0(t: Tensor) -> Tensor:
    out = 1.0 / t
    out[torch.isinf(out)] = 0
    return out


def generate_norm_HCHA(data, symdegnorm: bool = False, hyperedge_weight: Optional[Tensor] = None):
    """The scales ``HypergraphConv.forward`` derives from ``hyperedge_index`` on every call (reference layers.py:438-470), once:
    ``data.HCHA_D`` [N] = 1 / deg(v) (``symdegnorm``: deg(v)^-1/2), ``data.HCHA_B`` [M] = 1 / |e|, inf -> 0, float32 as in the
    reference; N = ``data.x`` rows (``data.n_x[0]`` without features), M = max hyperedge id + 1 after re-basing to 0.  With
    ``hyperedge_weight`` ([M]; None = ones) the degree is the weighted one, deg(v) = sum of ``w[e]`` over the hyperedges of ``v``; the
    weight enters ``D`` only, as in the reference."""
    num_nodes = data.x.shape[0] if getattr(data, 'x', None) is not None else _first(data.n_x)
    v, e, N, M = _vertex_edge_ids(data.edge_index, num_nodes)
    if hyperedge_weight is None:
        deg = torch.bincount(v, minlength=N).to(torch.float32)
    else:
        if hyperedge_weight.dim() != 1 or hyperedge_weight.numel() != M:
            raise ValueError(f"generate_norm_HCHA: hyperedge_weight has shape {tuple(hyperedge_weight.shape)}, expected ({M},)")
        w = hyperedge_weight.detach().to(device=v.device, dtype=torch.float32)
        deg = torch.zeros(N, dtype=torch.float32, device=v.device).index_add_(0, v, w[e])
    size = torch.bincount(e, minlength=M).to(torch.float32)
    data.HCHA_D = _inv0(deg.pow(0.5) if symdegnorm else deg)
    data.HCHA_B = _inv0(size)
    data.HCHA_symdegnorm = bool(symdegnorm)
    return data


def generate_norm_HNHN(H, data, args):
    """HNHN's normalisations (reference preprocessing.py:295-340) from the edge list; ``H`` (the reference's dense incidence matrix)
    is not used and may be None.  With beta = ``args.HNHN_beta``, alpha = ``args.HNHN_alpha``:
    ``D_v_beta = deg^beta``, ``D_e_beta_inv = 1 / sum_{v in e} deg(v)^beta``, ``D_e_alpha = |e|^alpha``,
    ``D_v_alpha_inv = 1 / sum_{e ni v} |e|^alpha`` (1/0 -> 0), computed in float64 and stored as float32.  Hyperedges are indexed by
    id - min id (what the model's propagate indexes them by) over max id + 1 entries."""
    alpha, beta = float(args.HNHN_alpha), float(args.HNHN_beta)
    v, e, N, M = _vertex_edge_ids(data.edge_index, _first(data.n_x))
    DV = torch.bincount(v, minlength=N).to(torch.float64)
    DE = torch.bincount(e, minlength=M).to(torch.float64)
    D_v_beta = DV.pow(beta)
    D_e_alpha = DE.pow(alpha)
    D_e_beta = torch.zeros(M, dtype=torch.float64, device=v.device).index_add_(0, e, D_v_beta[v])
    D_v_alpha = torch.zeros(N, dtype=torch.float64, device=v.device).index_add_(0, v, D_e_alpha[e])
    data.D_e_alpha = D_e_alpha.float()
    data.D_v_alpha_inv = _inv0(D_v_alpha).float()
    data.D_v_beta = D_v_beta.float()
    data.D_e_beta_inv = _inv0(D_e_beta).float()
    return data


# ---- UniGCNII (reference train.py:390-412, preprocessing.py:186-203) ----------------------------------------------------------------
def ConstructH_pairs(data):
    """The reference's ``ConstructH`` + ``torch_sparse.from_scipy(csr_matrix(H))`` without the dense 0/1 matrix: the (vertex, hyperedge)
    pairs of ``data.edge_index`` ([V; E], hyperedge ids anywhere) de-duplicated (a 0/1 matrix holds a repeated pair once), hyperedges
    renumbered 0..M-1 in the sorted order of the ids that occur, sorted by vertex then hyperedge.  Sets ``data.edge_index`` = the int64
    ``[V; E]`` pairs and ``data.UniGNN_sizes`` = ``(N, M)`` with N = ``data.x`` rows (vertices in no hyperedge keep their row, as
    H's zero rows do); returns ``data``."""
    ei = data.edge_index
    n = int(data.x.shape[0])
    if ei.numel() == 0:
        raise ValueError("ConstructH_pairs: the edge list is empty")
    if int(ei[0].min()) < 0 or int(ei[0].max()) >= n:
        raise ValueError(f"ConstructH_pairs: vertex ids span [{int(ei[0].min())}, {int(ei[0].max())}] but data.x has {n} rows")
    ids, e = torch.unique(ei[1], return_inverse=True)                 # sorted ids -> 0..M-1
    m = int(ids.numel())
    key = torch.unique(ei[0].to(torch.int64) * m + e)                 # sorted by (vertex, hyperedge), duplicates once
    data.edge_index = torch.stack([key // m, key % m]).contiguous()
    data.UniGNN_sizes = (n, m)
    return data


def generate_norm_UniGNN(data, args):
    """UniGCNII's degree scales (reference train.py:405-412) from the pairs of :func:`ConstructH_pairs`, in float32 as there:
    ``degV`` [N, 1] = (number of hyperedges of v)^-1/2 with inf -> 1 (a vertex in no hyperedge), ``degE`` [M, 1] = (mean over the
    members of e of their hyperedge counts)^-1/2; stored as ``args.UniGNN_degV`` / ``args.UniGNN_degE``.  Also
    ``data.UniGNN_scaleE`` [M] = ``degE / |e|``: the per-hyperedge scale that makes the V->E mean and the ``degE`` factor one
    ``scaled_propagate``.  Returns ``(degV, degE, scaleE)``."""
    if getattr(data, 'UniGNN_sizes', None) is None:
        raise ValueError("generate_norm_UniGNN: pass data through ConstructH_pairs first")
    n, m = data.UniGNN_sizes
    v, e = data.edge_index[0], data.edge_index[1]
    degV = torch.bincount(v, minlength=n).to(torch.float32)
    size = torch.bincount(e, minlength=m).to(torch.float32)
    degE = torch.zeros(m, dtype=torch.float32, device=v.device).index_add_(0, e, degV[v]) / size.clamp(min=1)
    degE = degE.pow(-0.5)
    degV = degV.pow(-0.5)
    degV[torch.isinf(degV)] = 1
    args.UniGNN_degV = degV.view(-1, 1)
    args.UniGNN_degE = degE.view(-1, 1)
    data.UniGNN_scaleE = degE / size
    return args.UniGNN_degV, args.UniGNN_degE, data.UniGNN_scaleE


def rebase_hyperedge_ids(data):
    """``data.edge_index[1] -= data.edge_index[1].min()`` (reference train.py:381,388), without modifying the tensor in place."""
    ei = data.edge_index
    if ei.numel():
        data.edge_index = torch.stack([ei[0], ei[1] - ei[1].min()]).contiguous()
    return data
