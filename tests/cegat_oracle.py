"""Float64 CPU restatement of the clique-expansion baseline CEGAT for the tests (reference models.py:131-183 over torch_geometric
1.6.3's GATConv): plain torch on index lists, sharing no code with the package.  Dropout is given as explicit per-element factors.

GATConv 1.6.3, as restated: ``xw = x @ W^T`` viewed ``[n, H, C]``; ``al = (xw * att_l).sum(-1)``, ``ar = (xw * att_r).sum(-1)``;
self-loops removed from the edge list and one loop appended for every vertex ``0..n-1``; per edge ``s -> t`` and head
``e = leaky_relu(al[s] + ar[t], 0.2)``; ``p = exp(e - max_t e) / (sum_t exp(e - max_t e) + 1e-16)`` over the edges into ``t``;
``out[t] = sum p * xw[s]``; heads concatenated or averaged; ``+ bias``."""
from __future__ import annotations

import torch

D64 = torch.float64
SOFTMAX_EPS = 1e-16


def attention_edges(ei, n):
    """``ei`` without its self-loops, then the loops ``0..n-1``."""
    keep = ei[0] != ei[1]
    loops = torch.arange(n, dtype=ei.dtype)
    return torch.cat([ei[:, keep], torch.stack([loops, loops])], dim=1)


def segment_softmax(e, index, n):
    """torch_geometric.utils.softmax of 1.6.3 over the entries sharing ``index``; ``e`` [E, H]."""
    H = e.shape[1]
    mx = torch.full((n, H), -float("inf"), dtype=e.dtype)
    mx = mx.scatter_reduce(0, index.unsqueeze(-1).expand(-1, H), e.detach(), reduce="amax", include_self=True)
    ex = torch.exp(e - mx[index])
    den = torch.zeros((n, H), dtype=e.dtype).index_add_(0, index, ex)
    return ex / (den[index] + SOFTMAX_EPS)


def gat_hop(x, al, ar, ei, n_t, heads, slope=0.2, concat=True, bias=None, act=None, mask=None, report=None):
    """The hop alone over the edges ``ei`` as given (``ei[0]`` sources, ``ei[1]`` targets): ``x`` [n_s, H*C], ``al`` [n_s, H],
    ``ar`` [n_t, H].  ``report`` (a dict): receives ``min_abs_logit`` = min |al[s] + ar[t]| over the edges (the distance of the
    nearest pre-activation from leaky_relu's kink) and ``p`` (the attention coefficients)."""
    H = heads
    C = x.shape[1] // H
    s, t = ei[0], ei[1]
    pre = al[s] + ar[t]
    e = torch.nn.functional.leaky_relu(pre, slope)
    p = segment_softmax(e, t, n_t)
    if report is not None:
        report["min_abs_logit"] = float(pre.detach().abs().min()) if pre.numel() else float("inf")
        report["p"] = p.detach()
    msg = x.view(-1, H, C)[s] * p.unsqueeze(-1)
    out = torch.zeros((n_t, H, C), dtype=x.dtype).index_add_(0, t, msg)
    out = out.reshape(n_t, H * C) if concat else out.mean(dim=1)
    if bias is not None:
        out = out + bias
    if act == "relu":
        out = torch.relu(out)
    if mask is not None:
        out = out * mask
    return out


def gat_conv(x, ei, sd, prefix, heads, concat=True, act=None, mask=None, report=None):
    """GATConv 1.6.3 with the parameters ``sd[prefix + 'lin_l.weight' | 'att_l' | 'att_r' | 'bias']`` over the raw edge list."""
    n = x.shape[0]
    W = sd[prefix + "lin_l.weight"]
    H = heads
    C = W.shape[0] // H
    xw = x @ W.t()
    xh = xw.view(n, H, C)
    al = (xh * sd[prefix + "att_l"]).sum(-1)
    ar = (xh * sd[prefix + "att_r"]).sum(-1)
    return gat_hop(xw, al, ar, attention_edges(ei, n), n, H, 0.2, concat, sd.get(prefix + "bias"), act, mask, report)


def batch_norm(x, sd, prefix, training, eps=1e-5):
    if training:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = sd[prefix + "running_mean"], sd[prefix + "running_var"]
    return (x - mean) / torch.sqrt(var + eps) * sd[prefix + "weight"] + sd[prefix + "bias"]


def cegat_forward(sd, x, ei, n_convs, heads, output_heads, masks=None, bn=False, training=False, reports=None):
    """Between convs: relu, the normalisation (``bn``: BatchNorm1d, else Identity), dropout (``masks``: explicit factors)."""
    for i in range(n_convs):
        last = i == n_convs - 1
        H = output_heads if last else (heads if i == 0 else 1)
        mask = None if (last or masks is None) else masks[i]
        rep = None
        if reports is not None:
            rep = {}
            reports.append(rep)
        if last or not bn:
            x = gat_conv(x, ei, sd, f"convs.{i}.", H, concat=not last, act=None if last else "relu", mask=mask, report=rep)
        else:
            x = gat_conv(x, ei, sd, f"convs.{i}.", H, act="relu", report=rep)
            x = batch_norm(x, sd, f"normalizations.{i}.", training)
            if mask is not None:
                x = x * mask
    return x


def dense_gat(x, ei, sd, prefix, heads, concat=True):
    """The same conv with a dense masked softmax over ``A + I`` (A[t, s] = 1 for an edge s -> t, s != t): checks
    :func:`attention_edges` + :func:`segment_softmax` + :func:`gat_hop`."""
    n = x.shape[0]
    W = sd[prefix + "lin_l.weight"]
    H = heads
    C = W.shape[0] // H
    xh = (x @ W.t()).view(n, H, C)
    al = (xh * sd[prefix + "att_l"]).sum(-1)
    ar = (xh * sd[prefix + "att_r"]).sum(-1)
    A = torch.zeros((n, n), dtype=torch.bool)
    A[ei[1], ei[0]] = True
    A[torch.arange(n), torch.arange(n)] = True
    logit = torch.nn.functional.leaky_relu(ar.unsqueeze(1) + al.unsqueeze(0), 0.2)         # [t, s, H]
    logit = logit.masked_fill(~A.unsqueeze(-1), -float("inf"))
    att = torch.softmax(logit, dim=1)
    out = torch.einsum("tsh,shc->thc", att, xh)
    out = out.reshape(n, H * C) if concat else out.mean(1)
    b = sd.get(prefix + "bias")
    return out if b is None else out + b
