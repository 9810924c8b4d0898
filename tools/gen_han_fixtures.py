"""Record the REFERENCE's HAN (reference DGL_HAN/model.py, imported live and read-only) on the cases of tests/han_cases.py into
tests/golden/baselines_han*.npz.  ``dgl`` is not installed, so ``dgl.nn.pytorch.GATConv`` is a stand-in put into ``sys.modules`` before
the import: tests/han_oracle.py's restatement of DGL 0.7.1's ``GATConv`` as a module.  The fixtures therefore pin the COMPOSITION
(HANLayer's stack, SemanticAttention, HAN's layer chain and ``predict``), the parameter creation order and the ``state_dict`` layout to the
reference's own classes; the ``GATConv`` itself is pinned only by the restatement of its documented formulas.  Regenerates byte for
byte: ``python tools/gen_han_fixtures.py`` (``--check``: compare with the committed files instead of writing).

What each case records: the layout and checksum of the reference's initial ``state_dict`` under ``torch.manual_seed``; in float64 with
the case's perturbed parameters: the logits, d(sum(logits * G))/dx and every parameter gradient, in eval mode or in training mode with
the case's explicit dropout factors; the smallest |pre-activation| of any conv (the leaky-relu kink margin)."""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import han_cases as hc  # noqa: E402
import han_oracle as orc  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HAN_DIR = os.path.join(ref_shim.REFERENCE_SRC, "DGL_HAN")


def available() -> bool:
    return os.path.isfile(os.path.join(HAN_DIR, "model.py"))


def reference_model_module():
    """The reference's DGL_HAN/model.py with the stand-in ``dgl.nn.pytorch.GATConv``."""
    for name in ("dgl", "dgl.nn", "dgl.nn.pytorch"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["dgl.nn.pytorch"].GATConv = orc.GATConvStandIn
    spec = importlib.util.spec_from_file_location("_ref_dgl_han_model", os.path.join(HAN_DIR, "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _put(arrays, key, t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.size <= hc.WHOLE_MAX:
        arrays[key] = a
        return
    flat = a.astype(np.float64).reshape(-1)
    idx = hc.sample_idx(key, flat.size)
    arrays[key + ":idx"], arrays[key + ":val"] = idx.astype(np.int64), flat[idx]
    arrays[key + ":sum"], arrays[key + ":abs"] = np.float64(flat.sum()), np.float64(np.abs(flat).sum())
    arrays[key + ":shape"] = np.array(a.shape, dtype=np.int64)


def reference_case(name, ref):
    c = hc.spec(name)
    x, pairs, n_v, n_e = hc.raw_data(c)
    n = n_v + n_e
    edges = hc.dense_metapath_edges(pairs, n_v, n_e)
    gs = [SimpleNamespace(src=torch.from_numpy(r), dst=torch.from_numpy(cc), n=n) for r, cc in edges]
    torch.manual_seed(c["seed"])
    model = ref.HAN(num_meta_paths=len(gs), in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=hc.DROPOUT)
    chk = hc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = hc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    model.train(c["train"])
    masks = hc.masks(c, [g.src.numel() for g in gs])
    report = []
    for l, layer in enumerate(model.layers):
        for i, conv in enumerate(layer.gat_layers):
            conv.report = report
            if masks is not None:
                conv.feat_keep, conv.edge_keep = (torch.from_numpy(m) for m in masks[l][i])
    xr = torch.from_numpy(x).clone().requires_grad_(True)
    out = model(gs, xr)
    G = torch.from_numpy(hc.cotangent(c, n))
    (out * G).sum().backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters()}
    return dict(chk=chk, spec=spec, out=out.detach(), grad_x=xr.grad.detach(), grads=grads, margin=min(report))


def build(file, ref) -> dict:
    arrays = {}
    for name in hc.FILES[file]:
        r = reference_case(name, ref)
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        arrays[f"{name}/margin"] = np.float64(r["margin"])
        for k in ("out", "grad_x"):
            _put(arrays, f"{name}/{k}", r[k])
        for k, g in r["grads"].items():
            _put(arrays, f"{name}/grad:{k}", g)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    ref = reference_model_module()
    for file in hc.FILES:
        arrays = build(file, ref)
        path = os.path.join(GOLDEN, file + ".npz")
        if a.check:
            got = hc.load(file)
            assert sorted(got) == sorted(arrays), file
            for k in arrays:
                assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), (file, k)
            print(f"{file}: matches")
        else:
            hc.write_npz(path, arrays)
            print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")
        for name in hc.FILES[file]:
            print(f"  {name}: kink margin {float(arrays[name + '/margin']):.3e}")


if __name__ == "__main__":
    main()
