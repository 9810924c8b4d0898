"""Float64 plain-torch restatement of the HAN baseline (reference DGL_HAN/model.py on DGL 0.7.1's ``GATConv``), test-only; it shares
no code with the package.  Dropout enters as explicit factors (0 or 1 / (1 - p)): per element of the conv's input, per (edge, head)
of the attention coefficients.

DGL 0.7.1 ``GATConv.forward`` (nn/pytorch/conv/gatconv.py), as HAN constructs it (no residual, bias, activation = elu), on a graph
whose edges are ``src -> dst`` (a multigraph: every edge is its own message):
    h      = feat_drop(feat)
    fs     = fc(h).view(N, H, C)                              (one shared fc: feat_src is feat_dst)
    el     = (fs * attn_l).sum(-1),  er = (fs * attn_r).sum(-1)                     [N, H]
    e      = leaky_relu(el[src] + er[dst], 0.2)                                     [E, H]
    a      = attn_drop(edge_softmax(graph, e))               softmax over the edges that share a ``dst``; no epsilon
    rst[t] = sum over edges into t of fs[src] * a            [N, H, C]
    rst    = rst + bias.view(1, H, C);  return elu(rst)
HANLayer stacks the flattened conv outputs of its metapath graphs at dim 1 and applies SemanticAttention:
    w = project(z).mean(0)  (project = Linear(D, 128) -> Tanh -> Linear(128, 1, no bias));  beta = softmax(w, dim 0);  sum_m beta_m z[:, m]
HAN: the layers in sequence, then ``predict`` (a Linear)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def gat_hop(src, dst, n, fs, el, er, bias, edge_keep=None, report=None):
    """The message passing of the conv from its transformed features ``fs`` [n, H * C] and logit terms ``el`` / ``er`` [n, H]: [n, H * C]."""
    H = el.shape[1]
    C = fs.shape[1] // H
    pre = el[src] + er[dst]
    if report is not None:
        report.append(float(pre.detach().abs().min()))
    e = F.leaky_relu(pre, 0.2)
    idx = dst.view(-1, 1).expand(-1, H)
    mx = torch.full((n, H), -float("inf"), dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax", include_self=True)
    ex = torch.exp(e - mx[dst])
    den = torch.zeros((n, H), dtype=e.dtype).index_add(0, dst, ex)
    a = ex / den[dst]
    if edge_keep is not None:
        a = a * edge_keep
    rst = torch.zeros((n, H, C), dtype=e.dtype).index_add(0, dst, fs.view(n, H, C)[src] * a.unsqueeze(-1))
    return F.elu(rst + bias.view(1, H, C)).reshape(n, H * C)


def gat_conv(src, dst, n, feat, W, attn_l, attn_r, bias, feat_keep=None, edge_keep=None, report=None):
    """[n, H * C].  ``attn_l`` / ``attn_r`` [1, H, C]; ``feat_keep`` like ``feat`` or None; ``edge_keep`` [E, H] or None."""
    H, C = attn_l.shape[1], attn_l.shape[2]
    h = feat if feat_keep is None else feat * feat_keep
    fs = (h @ W.t()).view(n, H, C)
    el, er = (fs * attn_l).sum(-1), (fs * attn_r).sum(-1)
    return gat_hop(src, dst, n, fs.reshape(n, H * C), el, er, bias, edge_keep, report)


def semantic_attention(z, W1, b1, w2):
    """``z`` [N, M, D]; ``W1`` [128, D], ``b1`` [128], ``w2`` [1, 128] -> [N, D]."""
    w = (torch.tanh(z @ W1.t() + b1) @ w2.t()).mean(0)            # [M, 1]
    beta = torch.softmax(w, dim=0)
    return (beta.unsqueeze(0) * z).sum(1)


def han_forward(sd, graphs, n, x, n_layers, masks=None, report=None):
    """Logits of HAN from a ``state_dict`` ``sd`` (float64 tensors).  ``graphs``: list of ``(src, dst)``; ``masks``: None (eval) or
    ``masks[l][i] = (feat_keep, edge_keep)`` for conv ``i`` of layer ``l``."""
    h = x
    for l in range(n_layers):
        zs = []
        for i, (src, dst) in enumerate(graphs):
            p = f"layers.{l}.gat_layers.{i}."
            fk, ek = masks[l][i] if masks is not None else (None, None)
            zs.append(gat_conv(src, dst, n, h, sd[p + "fc.weight"], sd[p + "attn_l"], sd[p + "attn_r"], sd[p + "bias"], fk, ek, report))
        q = f"layers.{l}.semantic_attention.project."
        h = semantic_attention(torch.stack(zs, dim=1), sd[q + "0.weight"], sd[q + "0.bias"], sd[q + "2.weight"])
    return h @ sd["predict.weight"].t() + sd["predict.bias"]


class GATConvStandIn(nn.Module):
    """The restatement as a module with DGL 0.7.1 ``GATConv``'s constructor order and initialisation, for code that does
    ``from dgl.nn.pytorch import GATConv``.  The graph is any object with ``src``, ``dst`` (int64 tensors) and ``n``.  Dropout: the
    explicit factors in ``feat_keep`` / ``edge_keep`` (set by the caller) in training mode, nothing in eval mode."""

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

    def forward(self, graph, feat):
        fk, ek = (self.feat_keep, self.edge_keep) if self.training else (None, None)
        out = gat_conv(graph.src, graph.dst, graph.n, feat, self.fc.weight, self.attn_l, self.attn_r, self.bias, fk, ek, self.report)
        return out.view(graph.n, self._num_heads, self._out_feats)
