"""Record the REFERENCE's heterogeneous HAN (reference DGL_HAN/model_hetero.py, imported live and read-only) on the cases of
tests/han_hetero_cases.py into tests/golden/baselines_han_hetero.npz.  ``dgl`` is not installed, so two stand-ins are put into
``sys.modules`` before the import -- the arrangement of tools/gen_han_fixtures.py: ``dgl.nn.pytorch.GATConv`` is tests/han_oracle.py's
restatement of DGL 0.7.1's ``GATConv`` as a module, and ``dgl.metapath_reachable_graph`` is tests/han_hetero_oracle.py's scipy
restatement.  The fixtures therefore pin the COMPOSITION (HANLayer's metapath cache and stack, SemanticAttention, HAN's layer chain and
``predict``), the parameter creation order and the ``state_dict`` layout to the reference's own classes.  Data only: the inputs, the typed
edge lists, the parameters, the logits and the gradients.  Regenerates byte for byte: ``python tools/gen_han_hetero_fixtures.py``
(``--check``: compare with the committed file instead of writing)."""
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

import han_hetero_cases as hc  # noqa: E402
import han_hetero_oracle as horc  # noqa: E402
import han_oracle as orc  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HAN_DIR = os.path.join(ref_shim.REFERENCE_SRC, "DGL_HAN")


def available() -> bool:
    return os.path.isfile(os.path.join(HAN_DIR, "model_hetero.py"))


def _reachable_stand_in(g, metapath):
    src, dst = horc.reachable_edges(g, list(metapath))
    _, _, s, d = horc.reachable_csr(g, list(metapath))
    assert s == d
    return SimpleNamespace(src=torch.from_numpy(src), dst=torch.from_numpy(dst), n=g.num_nodes[d])


def reference_model_module():
    """The reference's DGL_HAN/model_hetero.py with the two stand-ins."""
    for name in ("dgl", "dgl.nn", "dgl.nn.pytorch"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["dgl"].metapath_reachable_graph = _reachable_stand_in
    sys.modules["dgl.nn.pytorch"].GATConv = orc.GATConvStandIn
    spec = importlib.util.spec_from_file_location("_ref_dgl_han_model_hetero", os.path.join(HAN_DIR, "model_hetero.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_case(name, ref):
    c = hc.spec(name)
    x, edges, num_nodes = hc.raw_data(c)
    g = horc.TypedGraph(edges, num_nodes)
    n = num_nodes["paper"]
    torch.manual_seed(c["seed"])
    model = ref.HAN(meta_paths=hc.META_PATHS, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"],
                    dropout=hc.DROPOUT)
    chk = hc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = hc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    model.train(c["train"])
    n_edges = [horc.reachable_edges(g, mp)[0].size for mp in hc.META_PATHS]
    masks = hc.masks(c, n_edges)
    report = []
    for l, layer in enumerate(model.layers):
        for i, conv in enumerate(layer.gat_layers):
            conv.report = report
            if masks is not None:
                conv.feat_keep, conv.edge_keep = (torch.from_numpy(m) for m in masks[l][i])
    xr = torch.from_numpy(x).clone().requires_grad_(True)
    out = model(g, xr)
    (out * torch.from_numpy(hc.cotangent(c, n))).sum().backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters()}
    return dict(chk=chk, spec=spec, x=x, edges=edges, sd=sd, out=out.detach(), grad_x=xr.grad.detach(), grads=grads, margin=min(report))


def build(ref) -> dict:
    arrays = {}
    for name in hc.CASES:
        r = reference_case(name, ref)
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        arrays[f"{name}/margin"] = np.float64(r["margin"])
        arrays[f"{name}/x"] = r["x"]
        for (s, e, d), (src, dst) in r["edges"].items():
            arrays[f"{name}/edges:{s}|{e}|{d}"] = np.stack([src, dst])
        for k, v in r["sd"].items():
            arrays[f"{name}/param:{k}"] = v.numpy()
        for k in ("out", "grad_x"):
            arrays[f"{name}/{k}"] = r[k].numpy()
        for k, g in r["grads"].items():
            arrays[f"{name}/grad:{k}"] = g.numpy()
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    arrays = build(reference_model_module())
    path = os.path.join(GOLDEN, hc.FILE + ".npz")
    if a.check:
        got = hc.load(hc.FILE)
        assert sorted(got) == sorted(arrays)
        for k in arrays:
            assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), k
        print(f"{hc.FILE}: matches")
    else:
        hc.write_npz(path, arrays)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")
    for name in hc.CASES:
        print(f"  {name}: kink margin {float(arrays[name + '/margin']):.3e}")


if __name__ == "__main__":
    main()
