"""Record the REFERENCE's HCHA / HGNN / HNHN (reference models.py:207-292, layers.py:233-494, preprocessing.py:295-340, train.py:375-388)
on the cases of tests/baselines_cases.py into tests/golden/baselines_{hcha,hnhn,cora}.npz.  Container-only: imports the reference
through oracle/ref_shim.py (read-only).  Regenerates byte for byte: ``python tools/gen_baseline_fixtures.py`` (``--check``: compare
with the committed files instead of writing).

The shim's ``MessagePassing`` serves ``flow='source_to_target'`` only; ``HypergraphConv`` and ``HNHNConv`` switch ``self.flow`` to
``'target_to_source'`` for their E->V hop.  This file gives those two classes a flow-aware ``propagate`` (PyG 1.6.3 semantics:
``_j`` arguments gathered with ``edge_index[j]``, ``_i`` with ``edge_index[i]``, (i, j) = (1, 0) for source_to_target and (0, 1)
otherwise; messages summed into ``size[1]`` rows at ``edge_index[i]``) and checks it: the reference's first HCHA conv in float64
against the dense ``D^-1 H B^-1 H^T X Theta + b`` (and the symmetric form) before anything is recorded.

What each case records: the preprocessed ``edge_index`` and (HNHN) the four norms as the reference computed them; the checksum of
the reference's initial ``state_dict`` under ``torch.manual_seed``; in float64 with the case's perturbed parameters: logits,
d(sum(logits * G))/dx and every parameter gradient, in eval mode or in training mode with the case's explicit dropout factors
replacing ``F.dropout``.  HNHN without self-loops: the reference's ``ConstructH_HNHN`` reads ``data.totedges``, which only
``Add_Self_Loops`` sets; it is set to the raw hyperedge count here."""
from __future__ import annotations

import argparse
import inspect
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import baselines_cases as bc  # noqa: E402
from oracle import ref_shim  # noqa: E402


def _flow_propagate(self, edge_index, size=None, **kwargs):
    i, j = (1, 0) if self.flow == "source_to_target" else (0, 1)
    args = {}
    for name in inspect.signature(self.message).parameters:
        if name.endswith("_j"):
            args[name] = kwargs[name[:-2]].index_select(0, edge_index[j])
        elif name.endswith("_i"):
            args[name] = kwargs[name[:-2]].index_select(0, edge_index[i])
        else:
            args[name] = kwargs.get(name)
    msg = self.message(**args)
    n_out = size[1] if size is not None and size[1] is not None else int(edge_index[i].max()) + 1
    return msg.new_zeros((n_out,) + tuple(msg.shape[1:])).index_add_(0, edge_index[i], msg)


class _Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _reference():
    ref_layers, ref_models = ref_shim.import_reference()
    ref_pre = ref_shim.import_reference_preprocessing()
    ref_layers.HypergraphConv.propagate = _flow_propagate
    ref_layers.HNHNConv.propagate = _flow_propagate
    return ref_layers, ref_models, ref_pre


def reference_preprocess(c, ref_pre):
    """The reference's branch of train.py:375-388 on the case's raw data."""
    x, block, n_v, n_e = bc.raw_data(c)
    data = _Data(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e], x=torch.from_numpy(x))
    args = bc.args_of(c)
    data = ref_pre.ExtractV2E(data)
    if c["self_loops"]:
        data = ref_pre.Add_Self_Loops(data)
    if c["method"] == "HNHN":
        if not hasattr(data, "totedges"):
            data.totedges = n_e
        H = ref_pre.ConstructH_HNHN(data)
        data = ref_pre.generate_norm_HNHN(H, data, args)
    data.edge_index[1] -= data.edge_index[1].min()
    return data, args


def _dense_check(ref_layers):
    """The flow-aware propagate against the dense restatement of HypergraphConv (both normalisations)."""
    g = torch.Generator().manual_seed(5)
    n_v, n_e = 30, 12
    ei = torch.stack([torch.randint(0, n_v - 2, (60,), generator=g), torch.randint(0, n_e, (60,), generator=g)])
    ei = torch.unique(ei, dim=1)
    x = torch.randn(n_v, 5, generator=g, dtype=torch.float64)
    for sym in (False, True):
        conv = ref_layers.HypergraphConv(5, 3, sym).double()
        with torch.no_grad():
            conv.bias.normal_(generator=g)
        got = conv(x, ei)
        m = int(ei[1].max()) + 1
        H = torch.zeros(n_v, m, dtype=torch.float64)
        H[ei[0], ei[1]] = 1.0
        deg, size = H.sum(1), H.sum(0)
        Dv = torch.where(deg > 0, deg.pow(-0.5 if sym else -1.0), torch.zeros_like(deg))
        B = torch.where(size > 0, 1.0 / size, torch.zeros_like(size))
        xw = x @ conv.weight
        want = (Dv[:, None] * (H @ (B[:, None] * (H.t() @ (Dv[:, None] * xw))))) if sym else (Dv[:, None] * (H @ (B[:, None] * (H.t() @ xw))))
        torch.testing.assert_close(got, want + conv.bias, rtol=1e-12, atol=1e-12)


def reference_case(name, ref):
    ref_layers, ref_models, ref_pre = ref
    c = bc.spec(name)
    data, args = reference_preprocess(c, ref_pre)
    torch.manual_seed(c["seed"])
    model = (ref_models.HNHN if c["method"] == "HNHN" else ref_models.HCHA)(args)
    chk = bc.checksum(model.state_dict())
    spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
    sd = bc.perturb(model.state_dict(), c)
    model = model.double()
    model.load_state_dict(sd)
    xr = data.x.clone().requires_grad_(True)
    data.x = xr
    masks = [torch.from_numpy(m) for m in bc.masks(c)]
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
    G = torch.from_numpy(bc.cotangent(c, logits.shape[0]))
    (logits * G).sum().backward()
    out = dict(edge_index=data.edge_index.clone(), chk=chk, spec=spec, logits=logits.detach(), grad_x=xr.grad.detach(),
               grads={k: p.grad.detach() for k, p in model.named_parameters()}, masks=masks)
    if c["method"] == "HNHN":
        out["norms"] = {k: getattr(data, k).clone() for k in ("D_e_alpha", "D_v_alpha_inv", "D_v_beta", "D_e_beta_inv")}
    return out


def _put(arrays, key, t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    if a.size <= bc.WHOLE_MAX:
        arrays[key] = a
        return
    flat = a.astype(np.float64).reshape(-1)
    idx = bc.sample_idx(key, flat.size)
    arrays[key + ":idx"], arrays[key + ":val"] = idx.astype(np.int64), flat[idx]
    arrays[key + ":sum"], arrays[key + ":abs"] = np.float64(flat.sum()), np.float64(np.abs(flat).sum())
    arrays[key + ":shape"] = np.array(a.shape, dtype=np.int64)


def build(file, ref) -> dict:
    arrays = {}
    for name in bc.FILES[file]:
        r = reference_case(name, ref)
        arrays[f"{name}/edge_index"] = r["edge_index"].numpy().astype(np.int64)
        arrays[f"{name}/chk"] = np.array(r["chk"])
        arrays[f"{name}/spec"] = np.array([f"{k}|{list(s)}|{d}" for k, s, d in r["spec"]])
        for k in ("logits", "grad_x"):
            _put(arrays, f"{name}/{k}", r[k])
        for k, g in r["grads"].items():
            _put(arrays, f"{name}/grad:{k}", g)
        for k, v in r.get("norms", {}).items():
            arrays[f"{name}/norm:{k}"] = v.numpy()
    return arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixtures instead of writing them")
    a = ap.parse_args()
    ref = _reference()
    _dense_check(ref[0])
    for file in bc.FILES:
        arrays = build(file, ref)
        path = os.path.join(bc.GOLDEN, file + ".npz")
        if a.check:
            got = bc.load(file)
            assert sorted(got) == sorted(arrays), file
            for k in arrays:
                assert np.array_equal(got[k], np.asarray(arrays[k]), equal_nan=got[k].dtype.kind == "f"), (file, k)
            print(f"{file}: matches")
        else:
            bc.write_npz(path, arrays)
            print(f"{path}: {os.path.getsize(path)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
