"""Float64 restatement of the heterogeneous HAN (reference DGL_HAN/model_hetero.py on DGL 0.7.1), test-only; it shares no code with
the package.

Metapath reachability (``dgl.metapath_reachable_graph``, DGL 0.7.1 transform.py): with ``adj(etype)`` the scipy CSR whose rows are the
relation's sources and whose columns are its targets,
    adj = adj(e_1) * adj(e_2) * ... * adj(e_k);   adj = (adj != 0);   srcs, dsts = adj.nonzero()
and the new graph has the edges ``srcs -> dsts`` between the first relation's source type and the last one's destination type: one per
pair, no self-loop added or removed.  Here the pairs are returned in row-major order with ascending targets.

The GAT formulas are tests/han_oracle.py's.  The EMPTY-ROW RULE (``GATConv(allow_zero_in_degree=True)``): a target ``t`` without an
incoming edge takes part in no softmax and receives no message, so ``rst[t] = 0`` and the conv's output row is ``elu(0 + bias)``; its
gradient reaches ``bias`` only (nothing of ``fs``, ``el`` or ``er`` enters that row).  ``gat_hop`` below asserts the forward half on
every call."""
import numpy as np
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import han_oracle as orc


class TypedGraph:
    """``edges``: ``{(srctype, etype, dsttype): (src, dst)}`` of int64 numpy arrays; ``num_nodes``: ``{ntype: count}``."""

    def __init__(self, edges, num_nodes):
        self.edges = {k: (np.asarray(s, dtype=np.int64), np.asarray(d, dtype=np.int64)) for k, (s, d) in edges.items()}
        self.num_nodes = dict(num_nodes)
        self.by_name = {k[1]: k for k in self.edges}

    def adj(self, etype):
        s, _, d = rel = self.by_name[etype]
        src, dst = self.edges[rel]
        return sp.csr_matrix((np.ones(src.size), (src, dst)), shape=(self.num_nodes[s], self.num_nodes[d]))


def reachable_csr(g, metapath):
    """``(rowptr int64, col int64, srctype, dsttype)`` of the binarised product, columns ascending within a row."""
    adj = None
    for e in metapath:
        adj = g.adj(e) if adj is None else adj * g.adj(e)
    adj = sp.csr_matrix(adj != 0)
    adj.eliminate_zeros()
    adj.sort_indices()
    return adj.indptr.astype(np.int64), adj.indices.astype(np.int64), g.by_name[metapath[0]][0], g.by_name[metapath[-1]][2]


def reachable_edges(g, metapath):
    """``(src, dst)`` int64 numpy arrays in row-major order."""
    rowptr, col, _, _ = reachable_csr(g, metapath)
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr)), col


def csr_product(rowptr_a, col_a, rowptr_b, col_b, n_b, n_c):
    """``(rowptr, col)`` int64 of pattern(A B) for two CSRs given as numpy arrays (duplicate entries allowed)."""
    def mat(rowptr, col, n_rows, n_cols):
        rows = np.repeat(np.arange(n_rows), np.diff(rowptr))
        return sp.csr_matrix((np.ones(col.size), (rows, col)), shape=(n_rows, n_cols))
    c = sp.csr_matrix((mat(rowptr_a, col_a, rowptr_a.size - 1, n_b) * mat(rowptr_b, col_b, n_b, n_c)) != 0)
    c.eliminate_zeros()
    c.sort_indices()
    return c.indptr.astype(np.int64), c.indices.astype(np.int64)


def gat_hop(src, dst, n, fs, el, er, bias, edge_keep=None, report=None):
    """tests/han_oracle.py's hop on a graph that may have targets without incoming edges (and no edge at all)."""
    if src.numel() == 0:
        return F.elu(torch.zeros((n, fs.shape[1]), dtype=fs.dtype) + bias.view(1, -1))
    out = orc.gat_hop(src, dst, n, fs, el, er, bias, edge_keep, report)
    empty = torch.bincount(dst, minlength=n) == 0
    if bool(empty.any()):                                   # the empty-row rule
        assert torch.equal(out.detach()[empty], F.elu(bias.detach()).view(1, -1).expand(int(empty.sum()), -1))
    return out


def han_forward(sd, graphs, n, x, n_layers, masks=None, report=None):
    """tests/han_oracle.py's ``han_forward`` (the state_dict layout of model_hetero.py is model.py's) with the hop above."""
    h = x
    for l in range(n_layers):
        zs = []
        for i, (src, dst) in enumerate(graphs):
            p = f"layers.{l}.gat_layers.{i}."
            fk, ek = masks[l][i] if masks is not None else (None, None)
            H, C = sd[p + "attn_l"].shape[1], sd[p + "attn_l"].shape[2]
            hh = h if fk is None else h * fk
            fs = (hh @ sd[p + "fc.weight"].t()).view(n, H, C)
            el, er = (fs * sd[p + "attn_l"]).sum(-1), (fs * sd[p + "attn_r"]).sum(-1)
            zs.append(gat_hop(src, dst, n, fs.reshape(n, H * C), el, er, sd[p + "bias"], ek, report))
        q = f"layers.{l}.semantic_attention.project."
        h = orc.semantic_attention(torch.stack(zs, dim=1), sd[q + "0.weight"], sd[q + "0.bias"], sd[q + "2.weight"])
    return h @ sd["predict.weight"].t() + sd["predict.bias"]
