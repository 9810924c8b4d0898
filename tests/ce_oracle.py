"""Float64 CPU restatement of the clique-expansion baseline CEGCN for the tests (reference preprocessing.py:343-391 ConstructV2V,
norm_contruction TYPE='V2V' = torch_geometric 1.6.3 gcn_norm with self-loops, models.py:80-128 with GCNConv(normalize=False)):
plain torch / Python on index lists, sharing no code with the package.  Dropout is given as explicit per-element factors."""
from __future__ import annotations

from itertools import combinations

import torch

D64 = torch.float64


def clique_expansion(edge_index):
    """``[2, nnz]`` (vertex, hyperedge) -> (pairs int64 [2, E] sorted by (i, j), multiplicity float64 [E])."""
    members = {}
    for v, e in edge_index.t().tolist():
        members.setdefault(e, set()).add(v)
    count = {}
    for mem in members.values():
        for pair in combinations(sorted(mem), 2):
            count[pair] = count.get(pair, 0) + 1
    keys = sorted(count)
    pairs = torch.tensor(keys, dtype=torch.int64).reshape(-1, 2).t().contiguous()
    return pairs, torch.tensor([count[k] for k in keys], dtype=D64)


def gcn_norm(pairs, mult):
    """(edge_index [pairs | loops 0..N-1], w) with N = max id + 1."""
    n = int(pairs.max()) + 1
    loops = torch.arange(n)
    src, dst = torch.cat([pairs[0], loops]), torch.cat([pairs[1], loops])
    m = torch.cat([mult.to(D64), torch.ones(n, dtype=D64)])
    deg = torch.zeros(n, dtype=D64).index_add_(0, dst, m)
    dinv = deg.pow(-0.5)
    dinv[torch.isinf(dinv)] = 0
    return torch.stack([src, dst]), dinv[src] * m * dinv[dst]


def gcn_conv(x, ei, w, weight, bias, act=None, mask=None):
    xw = x @ weight
    out = torch.zeros((x.shape[0], weight.shape[1]), dtype=x.dtype).index_add_(0, ei[1], xw[ei[0]] * w.unsqueeze(-1))
    if bias is not None:
        out = out + bias
    if act == "relu":
        out = torch.relu(out)
    if mask is not None:
        out = out * mask
    return out


def batch_norm(x, sd, prefix, training, eps=1e-5):
    """BatchNorm1d: batch statistics (biased variance) in training mode, the running ones in eval."""
    if training:
        mean, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mean, var = sd[prefix + "running_mean"], sd[prefix + "running_var"]
    return (x - mean) / torch.sqrt(var + eps) * sd[prefix + "weight"] + sd[prefix + "bias"]


def cegcn_forward(sd, x, ei, w, n_convs, masks=None, bn=False, training=False):
    """Between convs: relu, the normalisation (``bn``: BatchNorm1d, else Identity), dropout (``masks``: explicit factors).
    ``sd``: convs.{i}.weight [in, out], convs.{i}.bias, normalizations.{i}.*."""
    for i in range(n_convs):
        last = i == n_convs - 1
        mask = None if (last or masks is None) else masks[i]
        if last or not bn:
            x = gcn_conv(x, ei, w, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], act=None if last else "relu", mask=mask)
        else:
            x = gcn_conv(x, ei, w, sd[f"convs.{i}.weight"], sd[f"convs.{i}.bias"], act="relu")
            x = batch_norm(x, sd, f"normalizations.{i}.", training)
            if mask is not None:
                x = x * mask
    return x


def dense_gcn(x, pairs, mult, weight, bias):
    """``D^-1/2 (A + I') D^-1/2 X W + b`` with the dense weighted adjacency (A[j, i] = m of pair (i, j)) and I' the identity on the
    ids < N = max id + 1 only: checks :func:`gcn_norm` + :func:`gcn_conv`."""
    n_x = x.shape[0]
    n = int(pairs.max()) + 1
    A = torch.zeros((n_x, n_x), dtype=D64)
    A.index_put_((pairs[1], pairs[0]), mult.to(D64), accumulate=True)
    A[torch.arange(n), torch.arange(n)] += 1.0
    deg = A.sum(1)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    return dinv[:, None] * A * dinv[None, :] @ (x @ weight) + bias
