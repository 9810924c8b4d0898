"""HyperGCN restated in float64 from the reference's table of contributions (reference utils.py:86-221, models.py:29-77), sharing no
code with ``allset_amd``: numpy for the structure, torch float64 autograd for the model.

For a hyperedge with members m_0..m_{k-1} (edge-list order) and projections p_i = Z[m_i] . rv: S = the member at the first arg-max,
I = at the first arg-min.  W (N x N) accumulates per hyperedge
    mediators, w = 1 / (2k - 3):  S != I: W[S,I], W[I,S] += w; every other member m: W[S,m], W[m,S], W[I,m], W[m,I] += w
                                  S == I (all p equal): W[S,S] += 2w; every other member m: W[S,m], W[m,S] += 2w
    no mediators, w = 1 / k:      S != I: W[S,I], W[I,S] += w;   S == I: W[S,S] += 2w
and A = D^-1/2 (W + I) D^-1/2 with D = rowsum(W + I).  Two forms: ``dense_A`` fills the N x N matrix entry by entry as the table
reads; ``triplets`` lists (row, col, value) contributions without any dictionary and ``sparse_apply`` scatters them."""
from __future__ import annotations

import numpy as np
import torch


def roles(Z: np.ndarray, rv: np.ndarray, members):
    """(S, I) per hyperedge (-1 for an empty one) and, per hyperedge, (gap_hi, gap_lo, scale): the distance of the extreme to the
    runner-up at both ends and max_i sum_j |Z[m_i, j]| rv_j (None where k < 2 or the end is an exact tie)."""
    S, I, gaps = [], [], []
    for mem in members:
        if not mem:
            S.append(-1), I.append(-1), gaps.append(None)
            continue
        p = Z[mem] @ rv
        s, i = int(np.argmax(p)), int(np.argmin(p))
        S.append(mem[s]), I.append(mem[i])
        if len(mem) < 2:
            gaps.append(None)
            continue
        srt = np.sort(p)
        scale = float((np.abs(Z[mem]) @ np.abs(rv)).max())
        gaps.append((float(srt[-1] - srt[-2]), float(srt[1] - srt[0]), scale))
    return np.array(S), np.array(I), gaps


def triplets(members, S, I, mediators: bool):
    """The contributions of the table as three flat lists (row, col, value); repeated (row, col) are meant to add up."""
    r, c, v = [], [], []

    def add(a, b, w):
        r.append(a), c.append(b), v.append(w)

    for e, mem in enumerate(members):
        k = len(mem)
        if k == 0:
            continue
        s, i = int(S[e]), int(I[e])
        if mediators:
            w = 1.0 / (2 * k - 3)
            if s != i:
                add(s, i, w), add(i, s, w)
                for m in mem:
                    if m != s and m != i:
                        add(s, m, w), add(m, s, w), add(i, m, w), add(m, i, w)
            else:
                add(s, s, 2 * w)
                for m in mem:
                    if m != s:
                        add(s, m, 2 * w), add(m, s, 2 * w)
        else:
            w = 1.0 / k
            if s != i:
                add(s, i, w), add(i, s, w)
            else:
                add(s, s, 2 * w)
    return np.array(r, dtype=np.int64), np.array(c, dtype=np.int64), np.array(v, dtype=np.float64)


def dense_A(n: int, members, S, I, mediators: bool):
    """(A, dinv): the N x N matrix written entry by entry."""
    W = np.zeros((n, n))
    for e, mem in enumerate(members):
        k = len(mem)
        if k == 0:
            continue
        s, i = int(S[e]), int(I[e])
        if mediators:
            w = 1.0 / (2 * k - 3)
            if s != i:
                W[s, i] += w
                W[i, s] += w
                for m in mem:
                    if m != s and m != i:
                        W[s, m] += w
                        W[m, s] += w
                        W[i, m] += w
                        W[m, i] += w
            else:
                W[s, s] += 2 * w
                for m in mem:
                    if m != s:
                        W[s, m] += 2 * w
                        W[m, s] += 2 * w
        else:
            w = 1.0 / k
            if s != i:
                W[s, i] += w
                W[i, s] += w
            else:
                W[s, s] += 2 * w
    M = W + np.eye(n)
    dinv = M.sum(1) ** -0.5
    return dinv[:, None] * M * dinv[None, :], dinv


def sparse_dinv(n: int, trip):
    r, _, v = trip
    D = np.ones(n)
    np.add.at(D, r, v)
    return D ** -0.5


def sparse_apply(n: int, trip, x: np.ndarray) -> np.ndarray:
    """A x from the triplets: scale, scatter-add, add the identity's share, scale."""
    r, c, v = trip
    dinv = sparse_dinv(n, trip)
    y = dinv[:, None] * x
    out = y.copy()
    np.add.at(out, r, v[:, None] * y[c])
    return dinv[:, None] * out


def forward(sd, x: torch.Tensor, members, n: int, L: int, fast: bool, mediators: bool, rvs, masks=(), train=False, margins=None,
            gaps=None, structures=None):
    """Logits in float64 (autograd through ``x`` and the parameters of ``sd``; A is a constant).  ``rvs``: the projection vectors in
    the order the reference draws them.  ``margins`` / ``gaps`` / ``structures``: lists that receive, per layer, the relu margin
    min |pre| / max_row |pre|, the projection gaps and (S, I, dinv)."""
    H = x
    A = None
    if fast:
        S, I, g = roles(x.detach().numpy(), np.asarray(rvs[0], dtype=np.float64), members)
        An, dinv = dense_A(n, members, S, I, mediators)
        A = torch.from_numpy(An)
        if gaps is not None:
            gaps.append(g)
        if structures is not None:
            structures.append((S, I, dinv))
    for i in range(L):
        HW = H @ sd[f"layers.{i}.W"]
        if not fast:
            S, I, g = roles(HW.detach().numpy(), np.asarray(rvs[i], dtype=np.float64), members)
            An, dinv = dense_A(n, members, S, I, mediators)
            A = torch.from_numpy(An)
            if gaps is not None:
                gaps.append(g)
            if structures is not None:
                structures.append((S, I, dinv))
        pre = A @ HW + sd[f"layers.{i}.bias"]
        if margins is not None:
            a = pre.detach().abs()
            margins.append(float((a / a.max(dim=1, keepdim=True).values.clamp(min=1e-300)).min()))
        H = torch.relu(pre)
        if i < L - 1 and train:
            H = H * masks[i]
    return H
