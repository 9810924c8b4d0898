"""Record the REFERENCE's plain UniGNN model (reference models.py:601-907) with each of its five convs behind the UniGCNII
preprocessing branch (train.py:390-412: ExtractV2E -> [Add_Self_Loops] -> ConstructH -> degV / degE) on the cases of
tests/unignn_cases.py into tests/golden/baselines_unignn*.npz.  Needs the reference's sources: imports its models and preprocessing
through oracle/ref_shim.py (read-only).  Regenerates byte for byte: ``python tools/gen_unignn_fixtures.py`` (``--check``: compare with
the committed files instead of writing).  The degree branch is tools/gen_unigcnii_fixtures.py's restatement of the driver's script text.

What each case records: the pairs ``V`` / ``E`` and the scales, the checksum and layout of the reference's initial ``state_dict`` under
``torch.manual_seed``; in float64 with the case's perturbed parameters: the output (log-probabilities; for a 'conv' case the conv's
output), d(sum(output * G))/dx and every parameter gradient (``att_v`` has none: recorded as absent), in eval mode or in training mode
with the case's explicit dropout factors (``input_drop`` / ``dropout`` are replaced at run time by modules that multiply with them).
Results only: the inputs are rebuilt from seeds by tests/unignn_cases.py."""
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

import unignn_cases as gc  # noqa: E402
from gen_ce_fixtures import _Data, _put  # noqa: E402
from gen_unigcnii_fixtures import _MaskDropout, _reference, degree_branch  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def reference_case(name, ref):
    ref_models, ref_pre = ref
    c = gc.spec(name)
    x, block, n_v, n_e = gc.raw_data(c)
    data = _Data(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e], x=torch.from_numpy(x))
    data = ref_pre.ExtractV2E(data)
    if c["self_loops"]:
        data = ref_pre.Add_Self_Loops(data)
    nnz_raw = data.edge_index.shape[1]
    data = ref_pre.ConstructH(data)
    V, E, degV, degE = degree_branch(np.asarray(data.edge_index))
    assert (V.numel() < nnz_raw) == c["dup"], (name, V.numel(), nnz_raw)             # the repeated incidence collapsed
    args = gc.args_of(c)
    args.degV, args.degE = degV, degE
    torch.manual_seed(c["seed"])
    if c["kind"] == "conv":
        model = ref_models.UniGATConv(args, c["F"], c["hidden"], heads=c["heads"], dropout=0.0, skip_sum=True)
    else:
        model = ref_models.UniGNN(args, nfeat=c["F"], nhid=c["hidden"], nclass=c["C"], nlayer=c["L"], nhead=c["heads"], V=V, E=E)
    chk = gc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = gc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    args.degV, args.degE = degV.double(), degE.double()
    xr = torch.from_numpy(x).clone().requires_grad_(True)
    model.train(c["train"])
    if c["kind"] == "conv":
        out = model(xr, V, E)
    else:
        masks = [torch.from_numpy(m) for m in gc.masks(c)]
        model.input_drop, model.dropout = _MaskDropout(masks[:1]), _MaskDropout(masks[1:])
        model.train(c["train"])
        out = model(xr)
        assert model.input_drop.used + model.dropout.used == len(masks), (name, len(masks))
    G = torch.from_numpy(gc.cotangent(c, out.shape[0]))
    (out * G).sum().backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters() if p.grad is not None}
    nograd = [k for k, p in model.named_parameters() if p.grad is None]
    return dict(V=V, E=E, degV=degV, degE=degE, chk=chk, spec=spec, out=out.detach(), grad_x=xr.grad.detach(), grads=grads, nograd=nograd)


def build(file, ref) -> dict:
    arrays = {}
    for name in gc.FILES[file]:
        r = reference_case(name, ref)
        arrays[f"{name}/pairs"] = torch.stack([r["V"], r["E"]]).numpy().astype(np.int32)
        arrays[f"{name}/degV"] = r["degV"].numpy()
        arrays[f"{name}/degE"] = r["degE"].numpy()
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        arrays[f"{name}/nograd"] = np.array(r["nograd"], dtype=str)
        for k in ("out", "grad_x"):
            _put(arrays, f"{name}/{k}", r[k])
        for k, g in r["grads"].items():
            _put(arrays, f"{name}/grad:{k}", g)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    ref = _reference()
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
