"""Record the REFERENCE's CEGAT (reference models.py:131-183) behind its preprocessing branch (train.py:354-357: ExtractV2E ->
ConstructV2V -> norm_contruction(TYPE='V2V')) on the cases of tests/cegat_cases.py into tests/golden/baselines_cegat*.npz.
Container-only: imports the reference through oracle/ref_shim.py (read-only).  Regenerates byte for byte:
``python tools/gen_cegat_fixtures.py`` (``--check``: compare with the committed files instead of writing).

The reference takes ``GATConv`` from torch_geometric 1.6.3, which the shim only stubs.  This file patches ``ref_models.GATConv``
with a stand-in that restates the 1.6.3 semantics -- ``lin_l = Linear(in, H * C, bias=False)`` and ``lin_r`` the same object,
``att_l`` / ``att_r`` [1, H, C], ``reset_parameters`` = glorot(lin_l.weight), glorot(lin_r.weight), glorot(att_l), glorot(att_r),
zeros(bias); forward: ``remove_self_loops`` + ``add_self_loops(num_nodes = x.size(0))``, ``leaky_relu(alpha_l[j] + alpha_r[i], 0.2)``,
``torch_geometric.utils.softmax`` (max-subtracted, denominator + 1e-16) over the target index, heads concatenated or averaged,
``+ bias`` -- and checks it in float64 against a dense masked softmax over ``A + I`` before anything is recorded (the
``gcn_norm`` stand-in of tools/gen_ce_fixtures.py serves the preprocessing).

What each case records: the V2V ``edge_index`` the model is given, the checksum and layout of the reference's initial ``state_dict``
under ``torch.manual_seed``; in float64 with the case's perturbed parameters: logits, d(sum(logits * G))/dx and every parameter
gradient, in eval mode or in training mode with the case's explicit dropout factors replacing ``F.dropout``."""
from __future__ import annotations

import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import cegat_cases as gc  # noqa: E402
from gen_ce_fixtures import _Data, _put, gcn_norm  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _glorot(t):
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))                                  # torch_geometric.nn.inits.glorot
    t.data.uniform_(-a, a)


# ---- torch_geometric 1.6.3 stand-in ------------------------------------------------------------------------------------------------
class GATConv(torch.nn.Module):
    def __init__(self, in_channels, out_channels, heads=1, concat=True, negative_slope=0.2, dropout=0.0, add_self_loops=True,
                 bias=True, **kwargs):
        super().__init__()
        assert dropout == 0.0, "the reference's CEGAT never sets attention dropout"
        self.heads, self.out_channels, self.concat, self.negative_slope = heads, out_channels, concat, negative_slope
        self.add_self_loops = add_self_loops
        self.lin_l = torch.nn.Linear(in_channels, heads * out_channels, bias=False)
        self.lin_r = self.lin_l
        self.att_l = torch.nn.Parameter(torch.Tensor(1, heads, out_channels))
        self.att_r = torch.nn.Parameter(torch.Tensor(1, heads, out_channels))
        if bias:
            self.bias = torch.nn.Parameter(torch.Tensor(heads * out_channels if concat else out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        _glorot(self.lin_l.weight)
        _glorot(self.lin_r.weight)
        _glorot(self.att_l)
        _glorot(self.att_r)
        if self.bias is not None:
            self.bias.data.fill_(0)

    def forward(self, x, edge_index):
        H, C = self.heads, self.out_channels
        x_l = x_r = self.lin_l(x).view(-1, H, C)
        alpha_l = (x_l * self.att_l).sum(dim=-1)
        alpha_r = (x_r * self.att_r).sum(dim=-1)
        N = x_l.size(0)
        if self.add_self_loops:
            edge_index = edge_index[:, edge_index[0] != edge_index[1]]
            loop = torch.arange(N, dtype=edge_index.dtype)
            edge_index = torch.cat([edge_index, torch.stack([loop, loop])], dim=1)
        j, i = edge_index[0], edge_index[1]
        alpha = torch.nn.functional.leaky_relu(alpha_l[j] + alpha_r[i], self.negative_slope)
        idx = i.unsqueeze(-1).expand(-1, H)
        amax = torch.full((N, H), -float("inf"), dtype=alpha.dtype).scatter_reduce(0, idx, alpha, reduce="amax")
        out = (alpha - amax[i]).exp()
        alpha = out / (torch.zeros((N, H), dtype=alpha.dtype).index_add_(0, i, out)[i] + 1e-16)
        out = torch.zeros((N, H, C), dtype=x.dtype).index_add_(0, i, x_l[j] * alpha.unsqueeze(-1))
        out = out.view(-1, H * C) if self.concat else out.mean(dim=1)
        return out + self.bias if self.bias is not None else out


def _reference():
    _, ref_models = ref_shim.import_reference()
    ref_pre = ref_shim.import_reference_preprocessing()
    ref_models.GATConv = GATConv
    ref_pre.gcn_norm = gcn_norm
    return ref_models, ref_pre


def _dense_check():
    """The stand-in against a dense masked softmax over A + I: loops in the input dropped and re-added, an isolated vertex."""
    g = torch.Generator().manual_seed(6)
    n = 24
    ei = torch.randint(0, n - 2, (2, 90), generator=g)
    ei = torch.unique(ei, dim=1)
    ei = torch.cat([ei, torch.tensor([[3, 5], [3, 5]])], dim=1)                      # loops already present
    x = torch.randn(n, 6, generator=g, dtype=torch.float64)
    for H, concat in ((1, True), (3, True), (2, False)):
        conv = GATConv(6, 4, heads=H, concat=concat).double()
        with torch.no_grad():
            conv.bias.normal_(generator=g)
        got = conv(x, ei)
        xh = conv.lin_l(x).view(n, H, 4)
        al, ar = (xh * conv.att_l).sum(-1), (xh * conv.att_r).sum(-1)
        A = torch.zeros(n, n, dtype=torch.bool)
        A[ei[1], ei[0]] = True
        A[torch.arange(n), torch.arange(n)] = True
        logit = torch.nn.functional.leaky_relu(ar.unsqueeze(1) + al.unsqueeze(0), 0.2).masked_fill(~A.unsqueeze(-1), -float("inf"))
        want = torch.einsum("tsh,shc->thc", torch.softmax(logit, dim=1), xh)
        want = (want.reshape(n, H * 4) if concat else want.mean(1)) + conv.bias
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
        iso = conv.lin_l(x)[n - 1].view(H, 4)                                       # isolated: a one-entry softmax, p = 1
        torch.testing.assert_close(got[n - 1], (iso.reshape(-1) if concat else iso.mean(0)) + conv.bias, rtol=1e-12, atol=1e-12)


def reference_case(name, ref):
    ref_models, ref_pre = ref
    c = gc.spec(name)
    x, block, n_v, n_e = gc.raw_data(c)
    data = _Data(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e], x=torch.from_numpy(x))
    data = ref_pre.ExtractV2E(data)
    data = ref_pre.ConstructV2V(data)
    data = ref_pre.norm_contruction(data, TYPE='V2V')
    args = gc.args_of(c)
    torch.manual_seed(c["seed"])
    model = ref_models.CEGAT(in_dim=args.num_features, hid_dim=args.MLP_hidden, out_dim=args.num_classes,
                             num_layers=args.All_num_layers, heads=args.heads, output_heads=args.output_heads, dropout=args.dropout,
                             Normalization=args.normalization)
    chk = gc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = gc.perturbed(model.state_dict(), c)                # (lin_l / lin_r: one tensor under two names)
    model = model.double()
    model.load_state_dict(sd)
    xr = data.x.clone().requires_grad_(True)
    data.x = xr
    masks = [torch.from_numpy(m) for m in gc.masks(c)]
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
    G = torch.from_numpy(gc.cotangent(c, logits.shape[0]))
    (logits * G).sum().backward()
    return dict(edge_index=data.edge_index.clone(), chk=chk, spec=spec, logits=logits.detach(), grad_x=xr.grad.detach(),
                grads={k: p.grad.detach() for k, p in model.named_parameters()})


def build(file, ref) -> dict:
    arrays = {}
    for name in gc.FILES[file]:
        r = reference_case(name, ref)
        arrays[f"{name}/edge_index"] = r["edge_index"].numpy().astype(np.int32)
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
    _dense_check()
    for file in gc.FILES:
        arrays = build(file, ref)
        path = os.path.join(GOLDEN, file + ".npz")
        if a.check:
            got = gc.load(file)
            assert sorted(got) == sorted(arrays), file
            for k in arrays:
                assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), (file, k)
            print(f"{file}: matches")
        else:
            gc.write_npz(path, arrays)
            print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
