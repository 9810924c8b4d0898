"""Float64 CPU restatement of the hypergraph-convolution baselines (reference layers.py:233-494, models.py:207-292,
preprocessing.py:295-340) for the tests: plain torch on index lists, sharing no code with the package or the reference shim.

Edge lists are ``[2, nnz]`` int64 with row 0 = vertex ids, row 1 = hyperedge ids (already re-based to 0).  Dropout is given as
explicit per-element factors (0 or 1 / (1 - p)), one [rows, width] tensor per dropout site, so that a training-mode forward of the
product can be replayed exactly."""
from __future__ import annotations

import numpy as np
import torch

D64 = torch.float64


def _inv0(t):
    out = 1.0 / t
    out[torch.isinf(out)] = 0
    return out


def sizes(edge_index, n_v):
    v, e = edge_index[0], edge_index[1]
    n_e = int(e.max()) + 1 if e.numel() else 0
    deg = torch.zeros(n_v, dtype=D64).index_add_(0, v, torch.ones(v.numel(), dtype=D64))
    card = torch.zeros(n_e, dtype=D64).index_add_(0, e, torch.ones(e.numel(), dtype=D64))
    return deg, card


def hcha_scales(edge_index, n_v, symdegnorm):
    deg, card = sizes(edge_index, n_v)
    D = _inv0(deg.sqrt()) if symdegnorm else _inv0(deg)
    return D, _inv0(card)


def hnhn_norms_dense(edge_index, n_v, alpha, beta):
    """The reference's formulas over a dense [N, M] incidence matrix (numpy, loops over columns / rows as in
    preprocessing.py:295-340), hyperedge columns indexed by id."""
    ei = np.asarray(edge_index)
    n_e = int(ei[1].max()) + 1
    H = np.zeros((n_v, n_e))
    H[ei[0], ei[1]] = 1.0
    with np.errstate(divide="ignore"):
        DV = H.sum(axis=1)
        DE = H.sum(axis=0)
        D_e_alpha = DE ** alpha
        D_v_alpha = np.array([np.sum(DE[np.where(H[i] == 1)[0]] ** alpha) for i in range(n_v)])
        D_v_beta = DV ** beta
        D_e_beta = np.array([np.sum(DV[np.where(H[:, j] == 1)[0]] ** beta) for j in range(n_e)])
        D_v_alpha_inv = 1.0 / D_v_alpha
        D_e_beta_inv = 1.0 / D_e_beta
    D_v_alpha_inv[np.isinf(D_v_alpha_inv)] = 0
    D_e_beta_inv[np.isinf(D_e_beta_inv)] = 0
    return dict(D_e_alpha=D_e_alpha, D_v_alpha_inv=D_v_alpha_inv, D_v_beta=D_v_beta, D_e_beta_inv=D_e_beta_inv)


def propagate(x, gather_ids, out_ids, n_out, r=None, s=None, bias=None, act=None, mask=None):
    """``y[t] = mask * act(s[t] * sum_{j: out_ids[j] == t} r[gather_ids[j]] * x[gather_ids[j]] + bias)``."""
    if r is not None:
        x = r.unsqueeze(-1) * x             # the whole matrix, as the reference scales it (inf * 0 at an isolated row -> NaN gradients)
    rows = x[gather_ids]
    y = torch.zeros((n_out, x.shape[1]), dtype=x.dtype).index_add_(0, out_ids, rows)
    if s is not None:
        y = s.unsqueeze(-1) * y
    if bias is not None:
        y = y + bias
    if act == "relu":
        y = torch.relu(y)
    elif act == "elu":
        y = torch.nn.functional.elu(y)
    if mask is not None:
        y = y * mask
    return y


def hypergraph_conv(x, edge_index, weight, bias, symdegnorm, act=None, mask=None):
    n_v = x.shape[0]
    v, e = edge_index[0], edge_index[1]
    n_e = int(e.max()) + 1
    D, B = hcha_scales(edge_index, n_v, symdegnorm)
    xw = x @ weight
    h = propagate(xw, v, e, n_e, r=D if symdegnorm else None, s=B)
    return propagate(h, e, v, n_v, s=D, bias=bias, act=act, mask=mask)


def hcha_forward(sd, x, edge_index, n_convs, symdegnorm, masks=None):
    """``sd``: name -> tensor (convs.{i}.weight [in, out], convs.{i}.bias); ``masks``: n_convs - 1 factors or None (eval)."""
    for i in range(n_convs):
        last = i == n_convs - 1
        x = hypergraph_conv(x, edge_index, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], symdegnorm,
                            act=None if last else "elu", mask=None if (last or masks is None) else masks[i])
    return x


def hnhn_conv(x, edge_index, norms, w1, b1, w2, b2, nonlinear, act=None, mask=None):
    n_v = x.shape[0]
    v, e = edge_index[0], edge_index[1]
    n_e = int(e.max()) + 1
    x = x @ w1.t() + b1
    h = propagate(x, v, e, n_e, r=norms["D_v_beta"], s=norms["D_e_beta_inv"], act="relu" if nonlinear else None)
    h = h @ w2.t() + b2
    return propagate(h, e, v, n_v, r=norms["D_e_alpha"], s=norms["D_v_alpha_inv"], act=act, mask=mask)


def hnhn_forward(sd, x, edge_index, norms, n_convs, nonlinear=True, masks=None):
    for i in range(n_convs):
        last = i == n_convs - 1
        x = hnhn_conv(x, edge_index, norms, sd[f"convs.{i}.weight_v2e.weight"], sd[f"convs.{i}.weight_v2e.bias"],
                      sd[f"convs.{i}.weight_e2v.weight"], sd[f"convs.{i}.weight_e2v.bias"], nonlinear,
                      act=None if last else "relu", mask=None if (last or masks is None) else masks[i])
    return x


def dense_hcha_conv(x, edge_index, weight, bias, symdegnorm):
    """``D^-1 H B^-1 H^T X Theta + b`` (or the symmetric form) with the dense incidence matrix: checks :func:`hypergraph_conv`."""
    n_v = x.shape[0]
    n_e = int(edge_index[1].max()) + 1
    H = torch.zeros((n_v, n_e), dtype=D64)
    H.index_put_((edge_index[0], edge_index[1]), torch.ones(edge_index.shape[1], dtype=D64), accumulate=True)
    D, B = hcha_scales(edge_index, n_v, symdegnorm)
    xw = x @ weight
    if symdegnorm:
        return torch.diag(D) @ H @ torch.diag(B) @ H.t() @ torch.diag(D) @ xw + bias
    return torch.diag(D) @ H @ torch.diag(B) @ H.t() @ xw + bias
