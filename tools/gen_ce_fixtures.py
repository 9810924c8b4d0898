"""Record the REFERENCE's CEGCN (reference models.py:80-128) and its preprocessing branch (train.py:354-357: ExtractV2E ->
ConstructV2V -> norm_contruction(TYPE='V2V'), preprocessing.py:343-469) on the cases of tests/ce_cases.py into
tests/golden/baselines_ce*.npz.  Container-only: imports the reference through oracle/ref_shim.py (read-only).  Regenerates byte
for byte: ``python tools/gen_ce_fixtures.py`` (``--check``: compare with the committed files instead of writing).

The reference takes ``GCNConv`` and ``gcn_norm`` from torch_geometric 1.6.3, which the shim only stubs.  This file patches
``ref_models.GCNConv`` and ``ref_pre.gcn_norm`` with stand-ins that restate the 1.6.3 semantics (``gcn_norm``:
``add_remaining_self_loops`` with fill 1 over ``N = edge_index.max() + 1``, in-degree by target, ``deg^-1/2[row] * w *
deg^-1/2[col]``, inf -> 0; ``GCNConv(normalize=False)``: ``weight`` [in, out] glorot, ``bias`` zeros, ``out = sum_{j -> i} w_ji
(x W)_j + bias`` over ``x.size(0)`` rows) and checks them in float64 against the dense ``D^-1/2 (A + I') D^-1/2 X W + b`` before
anything is recorded.

What each case records: the clique expansion as the reference built it (``pairs`` edge_index and multiplicity ``pair_norm``, in
its dict order), the normalised V2V graph (``edge_index``, ``norm``), the checksum and layout of the reference's initial
``state_dict`` under ``torch.manual_seed``; in float64 with the case's perturbed parameters: logits, d(sum(logits * G))/dx and every
parameter gradient, in eval mode or in training mode with the case's explicit dropout factors replacing ``F.dropout``."""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import ce_cases as cc  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


# ---- torch_geometric 1.6.3 stand-ins ---------------------------------------------------------------------------------------------
def gcn_norm(edge_index, edge_weight=None, num_nodes=None, improved=False, add_self_loops=True, dtype=None):
    fill_value = 2.0 if improved else 1.0
    if num_nodes is None:
        num_nodes = int(edge_index.max()) + 1
    if edge_weight is None:
        edge_weight = torch.ones((edge_index.size(1),), dtype=dtype)
    if add_self_loops:                                     # add_remaining_self_loops
        row, col = edge_index[0], edge_index[1]
        mask = row != col
        loop_weight = torch.full((num_nodes,), fill_value, dtype=edge_weight.dtype)
        inv = ~mask
        loop_weight[row[inv]] = edge_weight[inv]
        edge_weight = torch.cat([edge_weight[mask], loop_weight])
        loop_index = torch.arange(num_nodes, dtype=edge_index.dtype)
        edge_index = torch.cat([edge_index[:, mask], torch.stack([loop_index, loop_index])], dim=1)
    row, col = edge_index[0], edge_index[1]
    deg = torch.zeros(num_nodes, dtype=edge_weight.dtype).index_add_(0, col, edge_weight)
    dinv = deg.pow(-0.5)
    dinv.masked_fill_(dinv == float('inf'), 0)
    return edge_index, dinv[row] * edge_weight * dinv[col]


class GCNConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, improved=False, cached=False, add_self_loops=True, normalize=True, bias=True,
                 **kwargs):
        super().__init__()
        assert not normalize, "the reference's CEGCN builds GCNConv(normalize=False) only"
        self.weight = torch.nn.Parameter(torch.Tensor(in_channels, out_channels))
        self.bias = torch.nn.Parameter(torch.Tensor(out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        a = math.sqrt(6.0 / (self.weight.size(-2) + self.weight.size(-1)))          # torch_geometric.nn.inits.glorot
        self.weight.data.uniform_(-a, a)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def forward(self, x, edge_index, edge_weight=None):
        x = x @ self.weight
        w = torch.ones(edge_index.size(1), dtype=x.dtype) if edge_weight is None else edge_weight.to(x.dtype)
        out = x.new_zeros((x.size(0), x.size(1))).index_add_(0, edge_index[1], x.index_select(0, edge_index[0]) * w.view(-1, 1))
        return out + self.bias if self.bias is not None else out


class _Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _reference():
    _, ref_models = ref_shim.import_reference()
    ref_pre = ref_shim.import_reference_preprocessing()
    ref_models.GCNConv = GCNConv
    ref_pre.gcn_norm = gcn_norm
    return ref_models, ref_pre


def _dense_check(ref_pre):
    """The stand-ins (through the reference's own ConstructV2V / norm_contruction) against the dense form, with a trailing id that
    is in no pair and an interior one."""
    g = torch.Generator().manual_seed(5)
    n_v, n_e = 30, 14
    rows = []
    for e in range(n_e):
        k = 1 if e == 3 else int(torch.randint(2, 6, (1,), generator=g))
        mem = torch.randperm(n_v - 3, generator=g)[:k]
        mem = mem[mem != 9]
        rows += [(int(v), n_v + e) for v in mem]
    rows += [(0, n_v + n_e), (1, n_v + n_e)]
    v2e = torch.tensor(sorted(set(rows)), dtype=torch.int64).t()
    data = ref_pre.ConstructV2V(_Data(edge_index=v2e))
    pairs, mult = data.edge_index.clone(), data.norm.double().clone()
    data.norm = data.norm.double()
    data = ref_pre.norm_contruction(data, TYPE='V2V')
    x = torch.randn(n_v, 5, generator=g, dtype=torch.float64)
    conv = GCNConv(5, 3, normalize=False).double()
    with torch.no_grad():
        conv.bias.normal_(generator=g)
    got = conv(x, data.edge_index, data.norm)
    n = int(pairs.max()) + 1
    A = torch.zeros(n_v, n_v, dtype=torch.float64)
    A.index_put_((pairs[1], pairs[0]), mult, accumulate=True)
    A[torch.arange(n), torch.arange(n)] += 1.0
    deg = A.sum(1)
    dinv = torch.where(deg > 0, deg.pow(-0.5), torch.zeros_like(deg))
    want = (dinv[:, None] * A * dinv[None, :]) @ (x @ conv.weight) + conv.bias
    torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
    assert n < n_v - 2 and torch.equal(got[n:], conv.bias.expand(n_v - n, 3))     # trailing ids: the bias alone


def reference_case(name, ref):
    ref_models, ref_pre = ref
    c = cc.spec(name)
    x, block, n_v, n_e = cc.raw_data(c)
    data = _Data(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e], x=torch.from_numpy(x))
    data = ref_pre.ExtractV2E(data)
    data = ref_pre.ConstructV2V(data)
    pairs, pair_norm = data.edge_index.clone(), data.norm.clone()
    data = ref_pre.norm_contruction(data, TYPE='V2V')
    args = cc.args_of(c)
    torch.manual_seed(c["seed"])
    model = ref_models.CEGCN(in_dim=args.num_features, hid_dim=args.MLP_hidden, out_dim=args.num_classes,
                             num_layers=args.All_num_layers, dropout=args.dropout, Normalization=args.normalization)
    chk = cc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = cc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    xr = data.x.clone().requires_grad_(True)
    data.x = xr
    masks = [torch.from_numpy(m) for m in cc.masks(c)]
    F = ref_models.F
    orig = F.dropout
    used = []

    def dropout(t, p=0.5, training=True, inplace=False):
        if not training:
            return t
        m = masks[len(used)]
        used.append(1)
        return t * m
    model.train(c["train"])
    F.dropout = dropout
    try:
        logits = model(data)
    finally:
        F.dropout = orig
    assert len(used) == len(masks), (name, len(used), len(masks))
    G = torch.from_numpy(cc.cotangent(c, logits.shape[0]))
    (logits * G).sum().backward()
    return dict(pairs=pairs, pair_norm=pair_norm, edge_index=data.edge_index.clone(), norm=data.norm.clone(), chk=chk, spec=spec,
                logits=logits.detach(), grad_x=xr.grad.detach(),
                grads={k: p.grad.detach() for k, p in model.named_parameters()})


def _put(arrays, key, t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.size <= cc.WHOLE_MAX:
        arrays[key] = a
        return
    flat = a.astype(np.float64).reshape(-1)
    idx = cc.sample_idx(key, flat.size)
    arrays[key + ":idx"], arrays[key + ":val"] = idx.astype(np.int64), flat[idx]
    arrays[key + ":sum"], arrays[key + ":abs"] = np.float64(flat.sum()), np.float64(np.abs(flat).sum())
    arrays[key + ":shape"] = np.array(a.shape, dtype=np.int64)


def build(file, ref) -> dict:
    arrays = {}
    for name in cc.FILES[file]:
        r = reference_case(name, ref)
        arrays[f"{name}/pairs"] = r["pairs"].numpy().astype(np.int64)
        arrays[f"{name}/pair_norm"] = r["pair_norm"].numpy().astype(np.float32)
        arrays[f"{name}/edge_index"] = r["edge_index"].numpy().astype(np.int64)
        arrays[f"{name}/norm"] = r["norm"].numpy().astype(np.float32)
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        for k in ("logits", "grad_x"):
            _put(arrays, f"{name}/{k}", r[k])
        for k, g in r["grads"].items():
            _put(arrays, f"{name}/grad:{k}", g)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    ref = _reference()
    _dense_check(ref[1])
    for file in cc.FILES:
        arrays = build(file, ref)
        path = os.path.join(GOLDEN, file + ".npz")
        if a.check:
            got = cc.load(file)
            assert sorted(got) == sorted(arrays), file
            for k in arrays:
                assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), (file, k)
            print(f"{file}: matches")
        else:
            cc.write_npz(path, arrays)
            print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
