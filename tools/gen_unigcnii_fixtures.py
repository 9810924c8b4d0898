"""Record the REFERENCE's UniGCNII (reference models.py:911-996) behind its preprocessing branch (train.py:390-412: ExtractV2E ->
[Add_Self_Loops] -> ConstructH -> degV / degE) on the cases of tests/unigcnii_cases.py into tests/golden/baselines_unigcnii*.npz.
Container-only: imports the reference's models and preprocessing through oracle/ref_shim.py (read-only; its ``torch_scatter.scatter``
stand-in serves ``reduce='mean'`` and ``dim_size``).  Regenerates byte for byte: ``python tools/gen_unigcnii_fixtures.py``
(``--check``: compare with the committed files instead of writing).

The degree branch of the reference's driver is script text, not a function: it is restated here on the reference's own ``ConstructH``
output -- the non-zeros of the 0/1 matrix in row-major order (what ``torch_sparse.from_scipy(csr_matrix(H))`` returns), ``degV`` the
float32 row sums, ``degE = scatter(degV[V], E, reduce='mean')``, both ``.pow(-0.5)``, infinite ``degV`` set to 1 -- and checked against
the dense formulas before anything is recorded.

What each case records: the pairs ``V`` / ``E`` and the scales the model is given, the checksum and layout of the reference's initial
``state_dict`` under ``torch.manual_seed``; in float64 with the case's perturbed parameters: logits, d(sum(logits * G))/dx and every
parameter gradient, in eval mode or in training mode with the case's explicit dropout factors (the model's ``dropout`` module is
replaced at run time by one that multiplies with them in order)."""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import unigcnii_cases as uc  # noqa: E402
from gen_ce_fixtures import _Data, _put  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _reference():
    _, ref_models = ref_shim.import_reference()
    ref_pre = ref_shim.import_reference_preprocessing()
    return ref_models, ref_pre


class _MaskDropout(torch.nn.Module):
    """Stands in for the model's ``nn.Dropout``: the case's explicit factors, in call order (identity in eval mode)."""

    def __init__(self, masks):
        super().__init__()
        self.masks, self.used = masks, 0

    def forward(self, t):
        if not self.training:
            return t
        m = self.masks[self.used]
        self.used += 1
        return t * m


def degree_branch(H: np.ndarray):
    """Reference train.py:395-412 on ``ConstructH``'s matrix: ``(V, E, degV [N, 1] f32, degE [M, 1] f32)``."""
    scatter = sys.modules["torch_scatter"].scatter
    row, col = np.nonzero(H)                                                        # row-major: sorted by vertex, then hyperedge
    V, E = torch.from_numpy(row.astype(np.int64)), torch.from_numpy(col.astype(np.int64))
    degV = torch.from_numpy(np.asarray(H.sum(1))).view(-1, 1).float()
    degE = scatter(degV[V], E, dim=0, reduce='mean')
    degE = degE.pow(-0.5)
    degV = degV.pow(-0.5)
    degV[torch.isinf(degV)] = 1
    # the dense formulas
    Hd = torch.from_numpy(H).double()
    dv = Hd.sum(1)
    want_e = ((Hd.t() @ dv) / Hd.sum(0)).pow(-0.5)
    torch.testing.assert_close(degE.double().view(-1), want_e, rtol=1e-6, atol=0)
    torch.testing.assert_close(degV.double().view(-1), torch.where(dv > 0, dv.pow(-0.5), torch.ones_like(dv)), rtol=1e-6, atol=0)
    return V, E, degV, degE


def reference_case(name, ref):
    ref_models, ref_pre = ref
    c = uc.spec(name)
    x, block, n_v, n_e = uc.raw_data(c)
    data = _Data(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e], x=torch.from_numpy(x))
    data = ref_pre.ExtractV2E(data)
    if c["self_loops"]:
        data = ref_pre.Add_Self_Loops(data)
    nnz_raw = data.edge_index.shape[1]
    data = ref_pre.ConstructH(data)
    V, E, degV, degE = degree_branch(np.asarray(data.edge_index))
    assert (V.numel() < nnz_raw) == c["dup"], (name, V.numel(), nnz_raw)             # the repeated incidence collapsed
    args = uc.args_of(c)
    args.UniGNN_degV, args.UniGNN_degE = degV, degE
    torch.manual_seed(c["seed"])
    model = ref_models.UniGCNII(args, nfeat=args.num_features, nhid=args.MLP_hidden, nclass=args.num_classes,
                                nlayer=args.All_num_layers, nhead=args.heads, V=V, E=E)
    chk = uc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    groups = [[k for k, p in model.named_parameters() if any(p is q for q in grp)] for grp in (model.reg_params, model.non_reg_params)]
    sd = uc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    xr = torch.from_numpy(x).clone().requires_grad_(True)
    data.x = xr
    masks = [torch.from_numpy(m) for m in uc.masks(c)]
    model.dropout = _MaskDropout(masks)
    model.train(c["train"])
    logits = model(data)
    assert model.dropout.used == len(masks), (name, model.dropout.used, len(masks))
    G = torch.from_numpy(uc.cotangent(c, logits.shape[0]))
    (logits * G).sum().backward()
    return dict(V=V, E=E, degV=degV, degE=degE, chk=chk, spec=spec, groups=groups, logits=logits.detach(), grad_x=xr.grad.detach(),
                grads={k: p.grad.detach() for k, p in model.named_parameters()})


def build(file, ref) -> dict:
    arrays = {}
    for name in uc.FILES[file]:
        r = reference_case(name, ref)
        arrays[f"{name}/pairs"] = torch.stack([r["V"], r["E"]]).numpy().astype(np.int32)
        arrays[f"{name}/degV"] = r["degV"].numpy()
        arrays[f"{name}/degE"] = r["degE"].numpy()
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        arrays[f"{name}/reg_params"] = np.array(r["groups"][0])
        arrays[f"{name}/non_reg_params"] = np.array(r["groups"][1])
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
    for file in uc.FILES:
        arrays = build(file, ref)
        path = os.path.join(GOLDEN, file + ".npz")
        if a.check:
            got = uc.load(file)
            assert sorted(got) == sorted(arrays), file
            for k in arrays:
                assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), (file, k)
            print(f"{file}: matches")
        else:
            uc.write_npz(path, arrays)
            print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
