"""Float64 restatement of the UniGCNII baseline (reference models.py:911-996, train.py:390-412), written from its formulas and sharing
no code with allset_amd: the preprocessing through a dense 0/1 incidence matrix, the conv in a sparse (index_add) and in a dense
(matrix product) form, the model with explicit dropout factors.  Test-only; runs on the CPU.

Preprocessing.  ``H`` [N, M] has a 1 for every (vertex, hyperedge) pair that occurs (a repeated pair once), columns in the sorted
order of the hyperedge ids that occur; ``degV = rowsum(H)``, ``degE[e] = mean of degV over the members of e``; both to the power
-1/2, an infinite ``degV`` (a vertex in no hyperedge) becomes 1.

Conv (``beta_i = log(lamda / (i + 1) + 1)``, ``alpha`` = 0.1, ``lamda`` = 0.5):
    Xe = degE * mean_{v in e} x[v];   Xv = degV * sum_{e ni v} Xe[e];   use_norm: Xv = Xv * s, s = 1 / ||Xv||_row (inf -> 0), detached
    Xi = (1 - alpha) Xv + alpha x0;   out = (1 - beta) Xi + beta Xi W^T
Model: x = relu(L0(drop(x))); x0 = x; per conv: x = relu(conv(drop(x))); logits = L_last(drop(x)); dropout p = 0.2."""
from __future__ import annotations

import math

import torch

ALPHA, LAMDA, DROPOUT = 0.1, 0.5, 0.2


def dense_incidence(v2e: torch.Tensor, n_v: int) -> torch.Tensor:
    """``H`` float64 [n_v, M] of a [2, nnz] (vertex id, hyperedge id) list."""
    ids = sorted(set(int(e) for e in v2e[1]))
    col = {e: i for i, e in enumerate(ids)}
    H = torch.zeros(n_v, len(ids), dtype=torch.float64)
    for v, e in zip(v2e[0].tolist(), v2e[1].tolist()):
        H[v, col[e]] = 1.0
    return H


def degrees(H: torch.Tensor):
    """``(degV [N, 1], degE [M, 1])`` float64."""
    dv = H.sum(1)
    de = (H.t() @ dv) / H.sum(0)
    degV = dv.pow(-0.5)
    degV[torch.isinf(degV)] = 1.0
    return degV.view(-1, 1), de.pow(-0.5).view(-1, 1)


def pairs(H: torch.Tensor):
    """``(V, E)``: the non-zeros of ``H``, sorted by vertex then hyperedge."""
    nz = H.nonzero()
    return nz[:, 0].contiguous(), nz[:, 1].contiguous()


def v2e_mean(x, V, E, degE):
    M = degE.shape[0]
    cnt = torch.zeros(M, dtype=x.dtype).index_add_(0, E, torch.ones(E.shape[0], dtype=x.dtype)).clamp(min=1)
    return torch.zeros(M, x.shape[1], dtype=x.dtype).index_add_(0, E, x[V]) / cnt.view(-1, 1) * degE.view(-1, 1)


def hop(xe, x0, V, E, degV, alpha, use_norm, detach=True, report=None):
    """The E->V half with the initial residual: ``Xi``.  ``detach=False`` differentiates through the row norm (NOT what the model
    does: the tests use it to show that their comparison can tell the two apart)."""
    N = degV.shape[0]
    Xv = torch.zeros(N, xe.shape[1], dtype=xe.dtype).index_add_(0, V, xe[E]) * degV.view(-1, 1)
    if use_norm:
        nrm = (Xv.detach() if detach else Xv).norm(dim=1, keepdim=True)
        s = torch.where(nrm > 0, 1.0 / nrm.clamp(min=1e-300), torch.zeros_like(nrm))
        if report is not None:
            report["t"] = s.detach().reshape(-1)
        Xv = Xv * s
    return (1 - alpha) * Xv + alpha * x0


def conv(x, V, E, degV, degE, alpha, beta, x0, W, use_norm):
    Xi = hop(v2e_mean(x, V, E, degE), x0, V, E, degV, alpha, use_norm)
    return (1 - beta) * Xi + beta * (Xi @ W.t())


def conv_dense(x, H, degV, degE, alpha, beta, x0, W, use_norm):
    Xe = degE * ((H.t() @ x) / H.sum(0).clamp(min=1).view(-1, 1))
    Xv = degV * (H @ Xe)
    if use_norm:
        nrm = Xv.detach().norm(dim=1, keepdim=True)
        Xv = Xv * torch.where(nrm > 0, 1.0 / nrm.clamp(min=1e-300), torch.zeros_like(nrm))
    Xi = (1 - alpha) * Xv + alpha * x0
    return (1 - beta) * Xi + beta * (Xi @ W.t())


def _relu(t, reports):
    if reports is not None:
        a = t.detach().abs()
        rel = a / a.amax(dim=1, keepdim=True).clamp_min(1e-300)
        rel = rel[a != 0]
        reports.append(float(rel.min()) if rel.numel() else float("inf"))
    return torch.relu(t)


def forward(sd, x, V, E, degV, degE, nlayer, use_norm, masks=None, reports=None, H=None):
    """Logits of the model with the ``state_dict`` ``sd`` (``convs.0`` / ``convs.{1..nlayer}.W`` / ``convs.{nlayer+1}``).  ``masks``: the
    nlayer + 2 dropout factors of a training-mode forward ([N, F], then [N, d] each), None in eval mode.  ``reports``: a list that
    receives, per relu, the smallest non-zero ``|pre-activation| / (largest of its row)``.  ``H``: use the dense form of the conv."""
    it = iter(masks) if masks is not None else None
    drop = (lambda t: t * next(it)) if it is not None else (lambda t: t)
    x = _relu(drop(x) @ sd["convs.0.weight"].t() + sd["convs.0.bias"], reports)
    x0 = x
    for i in range(nlayer):
        beta = math.log(LAMDA / (i + 1) + 1)
        W = sd[f"convs.{i + 1}.W.weight"]
        x = drop(x)
        z = conv_dense(x, H, degV, degE, ALPHA, beta, x0, W, use_norm) if H is not None else \
            conv(x, V, E, degV, degE, ALPHA, beta, x0, W, use_norm)
        x = _relu(z, reports)
    out = drop(x) @ sd[f"convs.{nlayer + 1}.weight"].t() + sd[f"convs.{nlayer + 1}.bias"]
    if it is not None:
        assert next(it, None) is None, "more dropout masks than dropout sites"
    return out
