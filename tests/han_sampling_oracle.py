"""Float64 restatement of mini-batch HAN (reference DGL_HAN/train_sampling.py on DGL 0.7.1), test-only; it shares no code with the
package.  Two parts.

The model on BLOCKS.  A block has ``n_src`` source nodes of which the first ``n_dst`` are the targets, and edges ``src -> dst`` in
block-local ids.  DGL 0.7.1 ``GATConv.forward`` on a block, as ``train_sampling.HANLayer`` constructs it (no residual, bias, elu,
``allow_zero_in_degree=True``):
    h_src  = feat_drop(feat);  fs = fc(h_src).view(n_src, H, C);  feat_dst = fs[:n_dst]
    el     = (fs * attn_l).sum(-1)            [n_src, H]          er = (feat_dst * attn_r).sum(-1)      [n_dst, H]
    e      = leaky_relu(el[src] + er[dst], 0.2);  a = attn_drop(edge_softmax(e))   (over the edges into each target; no epsilon)
    rst[t] = sum over edges into t of fs[src] * a;  return elu(rst + bias.view(1, H, C))                [n_dst, H, C]
Dropout enters as explicit factors (0 or 1 / (1 - p)).  ``HANLayer`` stacks the flattened conv outputs at dim 1 and applies
SemanticAttention; ``HAN`` = that layer, then ``predict``.

The sampler, in numpy: ``k`` walks per seed (one uniform incident node of the other kind, one uniform incident node back; a seed
without out-edges terminates), the distinct endpoints, self-loops removed, one self-loop added, ``to_block`` with the seeds first.
DGL's own orders inside a block are hash-table orders; this restatement fixes them: neighbours ascending with the self-loop last,
non-seed source nodes ascending."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F


# ---- model -----------------------------------------------------------------------------------------------------------------------
def gat_hop(src, dst, n_src, n_dst, fs, el, er, bias, edge_keep=None, report=None):
    """``fs`` [n_src, H * C], ``el`` [n_src, H], ``er`` [n_dst, H] -> [n_dst, H * C]."""
    H = el.shape[1]
    C = fs.shape[1] // H
    pre = el[src] + er[dst]
    if report is not None:
        report.append(float(pre.detach().abs().min()))
    e = F.leaky_relu(pre, 0.2)
    idx = dst.view(-1, 1).expand(-1, H)
    mx = torch.full((n_dst, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax", include_self=True)
    ex = torch.exp(e - mx[dst])
    den = torch.zeros((n_dst, H), dtype=e.dtype).index_add(0, dst, ex)
    a = ex / den[dst]
    if edge_keep is not None:
        a = a * edge_keep
    rst = torch.zeros((n_dst, H, C), dtype=e.dtype).index_add(0, dst, fs.view(n_src, H, C)[src] * a.unsqueeze(-1))
    return F.elu(rst + bias.view(1, H, C)).reshape(n_dst, H * C)


def gat_conv(src, dst, n_src, n_dst, feat, W, attn_l, attn_r, bias, feat_keep=None, edge_keep=None, report=None):
    H, C = attn_l.shape[1], attn_l.shape[2]
    h = feat if feat_keep is None else feat * feat_keep
    fs = (h @ W.t()).view(n_src, H, C)
    el, er = (fs * attn_l).sum(-1), (fs[:n_dst] * attn_r).sum(-1)
    return gat_hop(src, dst, n_src, n_dst, fs.reshape(n_src, H * C), el, er, bias, edge_keep, report)


def semantic_attention(z, W1, b1, w2):
    w = (torch.tanh(z @ W1.t() + b1) @ w2.t()).mean(0)
    beta = torch.softmax(w, dim=0)
    return (beta.unsqueeze(0) * z).sum(1)


def han_forward(sd, blocks, h_list, masks=None, report=None):
    """Logits [n_dst, classes] from a ``state_dict`` of float64 tensors.  ``blocks``: objects with ``src``, ``dst`` (int64 tensors),
    ``n_src``, ``n_dst``; ``masks[i] = (feat_keep, edge_keep)`` for conv ``i`` or None."""
    zs = []
    for i, (b, h) in enumerate(zip(blocks, h_list)):
        p = f"layers.0.gat_layers.{i}."
        fk, ek = masks[i] if masks is not None else (None, None)
        zs.append(gat_conv(b.src, b.dst, b.n_src, b.n_dst, h, sd[p + "fc.weight"], sd[p + "attn_l"], sd[p + "attn_r"], sd[p + "bias"],
                           fk, ek, report))
    q = "layers.0.semantic_attention.project."
    h = semantic_attention(torch.stack(zs, dim=1), sd[q + "0.weight"], sd[q + "0.bias"], sd[q + "2.weight"])
    return h @ sd["predict.weight"].t() + sd["predict.bias"]


class GATConvStandIn(nn.Module):
    """The restatement as a module with DGL 0.7.1 ``GATConv``'s constructor order and initialisation, for code that does ``from
    dgl.nn.pytorch import GATConv`` and calls it on a block.  Dropout: the explicit factors in ``feat_keep`` / ``edge_keep`` (set by
    the caller) in training mode, nothing in eval mode."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0., attn_drop=0., negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False, bias=True):
        super().__init__()
        assert not residual and bias and activation is F.elu and negative_slope == 0.2
        self._num_heads, self._out_feats = num_heads, out_feats
        self.fc = nn.Linear(in_feats, out_feats * num_heads, bias=False)
        self.attn_l = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.attn_r = nn.Parameter(torch.FloatTensor(size=(1, num_heads, out_feats)))
        self.bias = nn.Parameter(torch.FloatTensor(size=(num_heads * out_feats,)))
        self.feat_keep = self.edge_keep = None
        self.report = None
        gain = nn.init.calculate_gain('relu')
        nn.init.xavier_normal_(self.fc.weight, gain=gain)
        nn.init.xavier_normal_(self.attn_l, gain=gain)
        nn.init.xavier_normal_(self.attn_r, gain=gain)
        nn.init.constant_(self.bias, 0)

    def forward(self, block, feat):
        fk, ek = (self.feat_keep, self.edge_keep) if self.training else (None, None)
        out = gat_conv(block.src, block.dst, block.n_src, block.n_dst, feat, self.fc.weight, self.attn_l, self.attn_r, self.bias, fk, ek,
                       self.report)
        return out.view(block.n_dst, self._num_heads, self._out_feats)


# ---- sampler ---------------------------------------------------------------------------------------------------------------------
def adjacency(pairs, n_v, n_e):
    """``(v2e, e2v)``: per vertex the sorted distinct hyperedges, per hyperedge the sorted distinct vertices (binarised)."""
    v2e, e2v = [set() for _ in range(n_v)], [set() for _ in range(n_e)]
    for v, e in zip(pairs[0].tolist(), pairs[1].tolist()):
        v2e[v].add(e)
        e2v[e].add(v)
    return [sorted(s) for s in v2e], [sorted(s) for s in e2v]


def walk(v2e, e2v, n_v, metapath, seed_node, rng):
    """One walk's endpoint in global ids, or -1.  ``metapath`` 0 = VEV (only vertex ids have out-edges), 1 = EVE (only hyperedges)."""
    n_e = len(e2v)
    if metapath == 0:
        if not (0 <= seed_node < n_v) or not v2e[seed_node]:
            return -1
        e = v2e[seed_node][int(rng.integers(len(v2e[seed_node])))]
        return e2v[e][int(rng.integers(len(e2v[e])))]
    if not (n_v <= seed_node < n_v + n_e) or not e2v[seed_node - n_v]:
        return -1
    v = e2v[seed_node - n_v][int(rng.integers(len(e2v[seed_node - n_v])))]
    return n_v + v2e[v][int(rng.integers(len(v2e[v])))]


def neighbour_rows(v2e, e2v, n_v, metapath, seeds, k, rng):
    """Per seed: the distinct endpoints of ``k`` walks other than -1 and the seed, ascending, then the seed (its one self-loop)."""
    rows = []
    for s in seeds:
        ends = {walk(v2e, e2v, n_v, metapath, int(s), rng) for _ in range(k)}
        rows.append(sorted(ends - {-1, int(s)}) + [int(s)])
    return rows


def to_block(rows, seeds):
    """``(src_ids, src, dst, n_src, n_dst)``: the seeds first, then the other distinct nodes ascending; edges in target-major order."""
    seeds = [int(s) for s in seeds]
    assert len(set(seeds)) == len(seeds)
    others = sorted({u for r in rows for u in r} - set(seeds))
    src_ids = seeds + others
    local = {g: i for i, g in enumerate(src_ids)}
    src = [local[u] for r in rows for u in r]
    dst = [t for t, r in enumerate(rows) for _ in r]
    return (np.array(src_ids, dtype=np.int64), np.array(src, dtype=np.int64), np.array(dst, dtype=np.int64), len(src_ids), len(seeds))


def endpoint_distribution(v2e, e2v, n_v, metapath, seed_node):
    """Exact ``{endpoint: P(endpoint | seed)}`` of one walk: ``P(u | s) = sum over the middle nodes m shared by s and u of
    1 / (deg(s) * deg(m))``; empty for a seed without out-edges."""
    n_e = len(e2v)
    first, second, base = (v2e, e2v, 0) if metapath == 0 else (e2v, v2e, n_v)
    loc = seed_node - base
    if not (0 <= loc < len(first)) or not first[loc]:
        return {}
    out = {}
    for m in first[loc]:
        for u in second[m]:
            out[u + base] = out.get(u + base, 0.0) + 1.0 / (len(first[loc]) * len(second[m]))
    assert abs(sum(out.values()) - 1.0) < 1e-12 and n_e >= 0
    return out
