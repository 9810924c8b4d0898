"""Float64 restatement of the hypergraph attention conv (reference layers.py:405-490, ``HypergraphConv(use_attention=True)``) and of
the attention HCHA model built from it, with explicit masks in place of every dropout.  Plain torch ops on whatever device the
inputs live on (the tests use the CPU); differentiable, so gradients come from autograd.

Incidences ``j = (v_j, e_j)`` in the order of the edge list ``ei`` ([2, nnz]: vertex ids, hyperedge ids)."""
from __future__ import annotations

import torch
import torch.nn.functional as F

SOFTMAX_EPS = 1e-16


def segment_softmax(src, index, n):
    """torch_geometric.utils.softmax (1.6.3): subtract the segment maximum, exponentiate, divide by (segment sum + 1e-16)."""
    H = src.shape[1]
    idx = index.view(-1, 1).expand(-1, H)
    mx = torch.full((n, H), float("-inf"), dtype=src.dtype).scatter_reduce(0, idx, src.detach(), reduce="amax", include_self=True)
    out = (src - mx[index]).exp()
    den = torch.zeros((n, H), dtype=src.dtype).index_add(0, index, out)
    return out / (den[index] + SOFTMAX_EPS)


def inv0(t):
    out = 1.0 / t
    return torch.where(torch.isinf(out), torch.zeros_like(out), out)


def scales(ei, n_v, n_e, hyperedge_weight=None, dtype=torch.float64):
    """``D[v] = 1 / sum_{e ni v} w[e]``, ``B[e] = 1 / |e|``; 0 where the sum is 0."""
    v, e = ei[0], ei[1]
    w = torch.ones(n_e, dtype=dtype) if hyperedge_weight is None else hyperedge_weight.to(dtype)
    D = inv0(torch.zeros(n_v, dtype=dtype).index_add(0, v, w[e]))
    B = inv0(torch.zeros(n_e, dtype=dtype).index_add(0, e, torch.ones(e.numel(), dtype=dtype)))
    return D, B


def act_fn(x, act):
    if act == "elu":
        return F.elu(x)
    if act == "relu":
        return torch.relu(x)
    assert act is None
    return x


def propagate(z, av, ae, ei, n_e, heads, D, B, slope=0.2, concat=True, bias=None, act=None, coef_mask=None, out_mask=None,
              softmax_by="vertex"):
    """Both hops under one coefficient.  ``coef_mask`` [nnz, H] and ``out_mask`` (the output's shape) hold ``keep / (1 - p)``.
    ``softmax_by='edge'`` normalises over the members of a hyperedge instead: NOT the layer's math (the sabotage test's variant)."""
    v, e = ei[0], ei[1]
    n_v = z.shape[0]
    C = z.shape[1] // heads
    zh = z.view(n_v, heads, C)
    logit = F.leaky_relu(av[v] + ae[e], slope)
    alpha = segment_softmax(logit, v, n_v) if softmax_by == "vertex" else segment_softmax(logit, e, n_e)
    a = alpha if coef_mask is None else alpha * coef_mask
    Y = torch.zeros((n_e, heads, C), dtype=z.dtype).index_add(0, e, a.unsqueeze(-1) * zh[v]) * B.view(-1, 1, 1)
    U = torch.zeros((n_v, heads, C), dtype=z.dtype).index_add(0, v, a.unsqueeze(-1) * Y[e]) * D.view(-1, 1, 1)
    out = U.reshape(n_v, heads * C) if concat else U.mean(dim=1)
    if bias is not None:
        out = out + bias
    out = act_fn(out, act)
    return out if out_mask is None else out * out_mask


def conv(x, weight, att, bias, ei, n_e, heads, slope=0.2, concat=True, hyperedge_weight=None, hyperedge_attr=None, act=None,
         coef_mask=None, out_mask=None, softmax_by="vertex"):
    """``HypergraphConv(use_attention=True)``.  ``hyperedge_attr``: None = the reference's ``z[hyperedge id]``; 'mean' = the mean of
    each hyperedge's member rows of ``x``; a tensor [n_e, in] = explicit edge-side rows."""
    n_v = x.shape[0]
    C = weight.shape[1] // heads
    z = x @ weight
    D, B = scales(ei, n_v, n_e, hyperedge_weight, x.dtype)
    if hyperedge_attr is None:
        assert n_e <= n_v
        ze = z[:n_e]
    elif isinstance(hyperedge_attr, str):
        assert hyperedge_attr == "mean"
        xe = torch.zeros((n_e, x.shape[1]), dtype=x.dtype).index_add(0, ei[1], x[ei[0]]) * B.view(-1, 1)
        ze = xe @ weight
    else:
        ze = hyperedge_attr @ weight
    av = (z.view(n_v, heads, C) * att[:, :, :C]).sum(-1)
    ae = (ze.view(n_e, heads, C) * att[:, :, C:]).sum(-1)
    return propagate(z, av, ae, ei, n_e, heads, D, B, slope, concat, bias, act, coef_mask, out_mask, softmax_by)


def plain_conv(x, weight, bias, ei, n_e, hyperedge_weight=None):
    """``HypergraphConv`` without attention (and without symdegnorm): ``D^-1 H B^-1 H^T X Theta + bias`` with the weighted ``D``."""
    D, B = scales(ei, x.shape[0], n_e, hyperedge_weight, x.dtype)
    z = x @ weight
    Y = torch.zeros((n_e, z.shape[1]), dtype=z.dtype).index_add(0, ei[1], z[ei[0]]) * B.view(-1, 1)
    U = torch.zeros_like(z).index_add(0, ei[0], Y[ei[1]]) * D.view(-1, 1)
    return U + bias if bias is not None else U


def hcha_forward(sd, x, ei, n_e, n_convs, heads, out_heads, coef_masks=None, out_masks=None):
    """The attention HCHA model: ``n_convs`` convs in 'mean' mode, ``elu`` (+ output mask) between them, heads concatenated on all but
    the last, which averages ``out_heads`` heads."""
    for i in range(n_convs):
        last = i == n_convs - 1
        x = conv(x, sd[f"convs.{i}.weight"], sd[f"convs.{i}.att"], sd[f"convs.{i}.bias"], ei, n_e, out_heads if last else heads,
                 concat=not last, hyperedge_attr="mean", act=None if last else "elu",
                 coef_mask=None if coef_masks is None else coef_masks[i],
                 out_mask=None if (last or out_masks is None) else out_masks[i])
    return x
