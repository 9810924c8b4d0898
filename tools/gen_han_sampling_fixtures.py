"""Record the REFERENCE's mini-batch HAN (reference DGL_HAN/train_sampling.py: its ``HAN`` and ``HANLayer``, imported live and
read-only) on the cases of tests/han_sampling_cases.py into tests/golden/baselines_han_sampling.npz.  ``dgl`` and ``ipdb`` are not
installed, so stand-ins go into ``sys.modules`` before the import: ``dgl.nn.pytorch.GATConv`` is tests/han_sampling_oracle.py's
restatement of DGL 0.7.1's ``GATConv`` on a block, everything else the reference's modules pull in (``dgl.sampling``,
``dgl.data.utils``, ``ipdb``) is a permissive stub that is never called.  The fixtures therefore pin the COMPOSITION (HANLayer's stack
over per-block inputs, SemanticAttention, ``predict``), the parameter creation order and the ``state_dict`` layout to the reference's own
classes; the ``GATConv`` itself and the sampler are pinned only by restatements of DGL's documented behaviour.  Regenerates byte for
byte: ``python tools/gen_han_sampling_fixtures.py`` (``--check``: compare with the committed file instead of writing).

What each case records: the layout and checksum of the reference's initial ``state_dict`` under ``torch.manual_seed``; in float64 with
the case's perturbed parameters on the case's fixed blocks: the logits, d(sum(logits * G))/d(input of each block) and every parameter
gradient, in eval mode or in training mode with explicit dropout factors; the smallest |pre-activation| of any conv."""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import han_sampling_cases as sc  # noqa: E402
import han_sampling_oracle as orc  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
HAN_DIR = os.path.join(ref_shim.REFERENCE_SRC, "DGL_HAN")


def available() -> bool:
    return os.path.isfile(os.path.join(HAN_DIR, "train_sampling.py"))


class _Permissive(types.ModuleType):
    """A module whose every attribute exists: a callable that refuses to be called (nothing recorded here goes through one)."""

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def _never(*a, **k):
            raise RuntimeError(f"{self.__name__}.{name} is a stand-in and must not be called")
        return _never


def reference_module():
    """The reference's DGL_HAN/train_sampling.py with the stand-ins; ``utils`` and ``model_hetero`` are the reference's own files,
    loaded under their plain names for the duration of the import only."""
    stubs = ["dgl", "dgl.nn", "dgl.nn.pytorch", "dgl.sampling", "dgl.data", "dgl.data.utils", "ipdb"]
    for name in ("scipy", "sklearn.metrics", "tqdm"):
        try:
            importlib.import_module(name)
        except ImportError:
            stubs.append(name)
            if "." in name:
                stubs.append(name.split(".")[0])
    saved = {k: sys.modules.get(k) for k in stubs + ["utils", "model_hetero"]}
    try:
        for name in stubs:
            sys.modules[name] = _Permissive(name)
        sys.modules["dgl.nn.pytorch"].GATConv = orc.GATConvStandIn
        for name in ("utils", "model_hetero"):
            sys.modules.pop(name, None)
        sys.path.insert(0, HAN_DIR)
        try:
            spec = importlib.util.spec_from_file_location("_ref_dgl_han_train_sampling", os.path.join(HAN_DIR, "train_sampling.py"))
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        finally:
            sys.path.remove(HAN_DIR)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def _put(arrays, key, t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.size <= sc.WHOLE_MAX:
        arrays[key] = a
        return
    flat = a.astype(np.float64).reshape(-1)
    idx = sc.sample_idx(key, flat.size)
    arrays[key + ":idx"], arrays[key + ":val"] = idx.astype(np.int64), flat[idx]
    arrays[key + ":sum"], arrays[key + ":abs"] = np.float64(flat.sum()), np.float64(np.abs(flat).sum())
    arrays[key + ":shape"] = np.array(a.shape, dtype=np.int64)


def reference_case(name, ref):
    c = sc.spec(name)
    x, pairs, n_v, n_e = sc.raw_data(c)
    blks = sc.blocks(c, pairs)
    torch.manual_seed(c["seed"])
    model = ref.HAN(num_metapath=len(blks), in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"],
                    dropout=sc.DROPOUT)
    chk = sc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = sc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    model.train(c["train"])
    masks = sc.masks(c, blks)
    report = []
    for i, conv in enumerate(model.layers[0].gat_layers):
        conv.report = report
        if masks is not None:
            conv.feat_keep, conv.edge_keep = (torch.from_numpy(m) for m in masks[i])
    xt = torch.from_numpy(x)
    hs = [xt[b.src_ids].clone().requires_grad_(True) for b in blks]
    out = model(blks, hs)
    (out * torch.from_numpy(sc.cotangent(c))).sum().backward()
    grads = {k: p.grad.detach() for k, p in model.named_parameters()}
    assert min(report) > sc.KINK_MARGIN, (name, min(report))
    return dict(chk=chk, spec=spec, out=out.detach(), grad_h=[h.grad.detach() for h in hs], grads=grads, margin=min(report))


def build(ref) -> dict:
    arrays = {}
    for name in sc.CASES:
        r = reference_case(name, ref)
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        arrays[f"{name}/margin"] = np.float64(r["margin"])
        _put(arrays, f"{name}/out", r["out"])
        for i, g in enumerate(r["grad_h"]):
            _put(arrays, f"{name}/grad_h{i}", g)
        for k, g in r["grads"].items():
            _put(arrays, f"{name}/grad:{k}", g)
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    arrays = build(reference_module())
    path = os.path.join(GOLDEN, sc.FILE + ".npz")
    if a.check:
        got = sc.load(sc.FILE)
        assert sorted(got) == sorted(arrays), sc.FILE
        for k in arrays:
            assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), (sc.FILE, k)
        print(f"{sc.FILE}: matches")
    else:
        sc.write_npz(path, arrays)
        print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")
    for name in sc.CASES:
        print(f"  {name}: kink margin {float(arrays[name + '/margin']):.3e}")


if __name__ == "__main__":
    main()
