"""Float64 restatement of the plain UniGNN model and its five convs (reference models.py:601-907), written from their formulas and
sharing no code with allset_amd or the reference.  Test-only; runs on the CPU.

With ``agg`` the sum or the mean (count clamped at 1) of the rows an index points to:
    UniGCN :  X = X W^T;  Xe = degE * agg1_{v in e} X[v];  Xv = degV * sum_{e ni v} Xe[e];  norm
    UniGCN2:  the same two hops and the norm on X itself, then  X W^T + b
    UniGIN :  X = X W^T;  Xe = agg1 X;  out = (1 + eps) X + sum Xe;  norm
    UniSAGE:  X = X W^T;  Xe = agg1 X;  out = X + agg2 Xe;  norm
    UniGAT :  X0 = X W^T as [N, H, C];  Xe = agg1 X0;  a[e, h] = <Xe[e, h], att_e[h]>;  per vertex and head
              p = softmax over its hyperedges of leaky_relu(a, 0.2)  (exp(. - max) / (sum + 1e-16));  out = sum p Xe;  norm;
              + X0 under skip_sum
norm (``use_norm``): every row times 1 / ||row||_2 taken from the DETACHED row, 0 for a zero row.
Model: x = drop_in(x); per hidden conv x = drop(act(conv(x))); log_softmax(conv_out(x))."""
from __future__ import annotations

import torch

SOFTMAX_EPS = 1e-16


def agg(rows, index, n, how):
    out = torch.zeros(n, *rows.shape[1:], dtype=rows.dtype).index_add_(0, index, rows)
    if how == "mean":
        cnt = torch.zeros(n, dtype=rows.dtype).index_add_(0, index, torch.ones(index.shape[0], dtype=rows.dtype)).clamp(min=1)
        out = out / cnt.view(-1, *([1] * (rows.dim() - 1)))
    return out


def row_norm(X, detach=True, report=None):
    nrm = (X.detach() if detach else X).norm(dim=1, keepdim=True)
    s = torch.where(nrm > 0, 1.0 / nrm.clamp(min=1e-300), torch.zeros_like(nrm))
    if report is not None:
        report["t"] = s.detach().reshape(-1)
    return X * s


def hop(xe, V, E, N, s=None, xs=None, c=1.0, use_norm=False, act=None, mask=None, detach=True, report=None, self_after_norm=False):
    """The E->V sum hop with its row tail: ``drop(act(norm(s * sum xe + c * xs)))``.  ``self_after_norm``: the WRONG order (self term
    added behind the norm), for the test that shows the comparison tells the two apart."""
    a = agg(xe[E], V, N, "sum")
    if s is not None:
        a = a * s.view(-1, 1)
    if xs is not None and not self_after_norm:
        a = a + c * xs
    if use_norm:
        a = row_norm(a, detach, report)
    if xs is not None and self_after_norm:
        a = a + c * xs
    if act == "relu":
        a = torch.relu(a)
    return a if mask is None else a * mask


def edge_logits(x, V, E, M, s, att, heads):
    xe = agg(x[V], E, M, "sum")
    if s is not None:
        xe = xe * s.view(-1, 1)
    ae = (xe.view(M, heads, -1) * att.reshape(1, heads, -1)).sum(-1)
    return xe, ae


def attention_pool(xe, ae, V, E, N, heads, slope=0.2):
    a = torch.nn.functional.leaky_relu(ae, slope)[E]                       # [nnz, H]
    mx = torch.full((N, heads), -float("inf"), dtype=a.dtype).scatter_reduce(0, V.view(-1, 1).expand(-1, heads), a.detach(), "amax")
    ex = (a - mx[V]).exp()
    den = torch.zeros(N, heads, dtype=a.dtype).index_add_(0, V, ex) + SOFTMAX_EPS
    p = ex / den[V]
    return agg((xe[E].view(-1, heads, xe.shape[1] // heads) * p.unsqueeze(-1)).reshape(E.shape[0], -1), V, N, "sum")


def conv(kind, P, x, V, E, degV, degE, cfg, logit_report=None, skip_sum=False):
    """``P``: the conv's parameters (``W.weight``, ``W.bias``, ``eps``, ``att_e``); ``cfg``: first, second, use_norm, heads."""
    N, M = degV.shape[0], degE.shape[0]
    first, use_norm = cfg["first"], cfg["use_norm"]
    W = P["W.weight"]
    if kind == "UniGCN":
        xe = agg((x @ W.t())[V], E, M, first) * degE.view(-1, 1)
        return hop(xe, V, E, N, s=degV.view(-1), use_norm=use_norm)
    if kind == "UniGCN2":
        xe = agg(x[V], E, M, first) * degE.view(-1, 1)
        return hop(xe, V, E, N, s=degV.view(-1), use_norm=use_norm) @ W.t() + P["W.bias"]
    if kind == "UniGIN":
        x = x @ W.t()
        return hop(agg(x[V], E, M, first), V, E, N, xs=x, c=1 + P["eps"], use_norm=use_norm)
    if kind == "UniSAGE":
        x = x @ W.t()
        xv = agg(agg(x[V], E, M, first)[E], V, N, cfg["second"])
        out = x + xv
        return row_norm(out) if use_norm else out
    if kind == "UniGAT":
        H = cfg["heads"]
        x0 = x @ W.t()
        xe = agg(x0[V], E, M, first)
        ae = (xe.view(M, H, -1) * P["att_e"].reshape(1, H, -1)).sum(-1)
        if logit_report is not None:
            a = ae.detach().abs()
            rel = a / a.max().clamp_min(1e-300)
            logit_report.append(float(rel[a != 0].min()) if bool((a != 0).any()) else float("inf"))
        out = attention_pool(xe, ae, V, E, N, H)
        if use_norm:
            out = row_norm(out)
        return out + x0 if skip_sum else out
    raise ValueError(kind)


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def forward(sd, x, V, E, degV, degE, cfg, masks=None, reports=None):
    """Log-probabilities of ``UniGNN`` with the ``state_dict`` ``sd``.  ``cfg``: model, L, heads, first, second, use_norm, activation.
    ``masks``: the L dropout factors of a training-mode forward (input, then one per hidden conv).  ``reports``: a list receiving, per
    relu, the smallest non-zero ``|pre-activation| / (largest of its row)`` and, per UniGAT conv, the same for the logits against the
    largest of the matrix."""
    it = iter(masks) if masks is not None else None
    drop = (lambda t: t * next(it)) if it is not None else (lambda t: t)
    x = drop(x)
    heads = cfg["heads"]
    for i in range(cfg["L"] - 1):
        z = conv(cfg["model"], _sub(sd, f"convs.{i}."), x, V, E, degV, degE, dict(cfg, heads=heads), reports)
        if cfg["activation"] == "relu":
            if reports is not None:
                a = z.detach().abs()
                rel = (a / a.amax(dim=1, keepdim=True).clamp_min(1e-300))[a != 0]
                reports.append(float(rel.min()) if rel.numel() else float("inf"))
            z = torch.relu(z)
        else:
            z = torch.where(z >= 0, z, z * sd["act.weight"])
        x = drop(z)
    out = conv(cfg["model"], _sub(sd, "conv_out."), x, V, E, degV, degE, dict(cfg, heads=1), reports)
    if it is not None:
        assert next(it, None) is None, "more dropout masks than dropout sites"
    return torch.log_softmax(out, dim=1)
