"""Record the REFERENCE's ``HypergraphConv(use_attention=True)`` (reference layers.py:318-494) on the cases of
tests/hcha_attn_cases.py into tests/golden/baselines_hcha_attn.npz.  Container-only: imports the reference through
oracle/ref_shim.py (read-only), with the flow-aware ``propagate`` of tools/gen_baseline_fixtures.py (the conv switches ``self.flow``
for its E->V hop).  Regenerates byte for byte: ``python tools/gen_hcha_attn_fixtures.py`` (``--check``: compare with the committed
file instead of writing).

What each case records: the checksum and the key / shape list of the reference layer's initial ``state_dict`` under
``torch.manual_seed``; in float64 with the case's perturbed parameters: the output, d(sum(out * G))/dx and every parameter gradient,
in eval mode or -- one case -- in training mode with the case's explicit [nnz, heads] factors replacing ``F.dropout`` on the
coefficients."""
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

import hcha_attn_cases as hc  # noqa: E402
from gen_baseline_fixtures import _flow_propagate  # noqa: E402
from oracle import ref_shim  # noqa: E402


def reference_case(name, ref_layers):
    c = hc.spec(name)
    x, ei, w = hc.inputs(c)
    torch.manual_seed(c["seed"])
    conv = ref_layers.HypergraphConv(hc.F_IN, c["out"], use_attention=True, heads=c["heads"], concat=c["concat"],
                                     dropout=hc.ATTN_DROP if c["train"] else 0)
    sd0 = conv.state_dict()
    chk = hc.checksum(sd0)
    keys = [f"{k}:{'x'.join(str(s) for s in v.shape)}" for k, v in sd0.items()]
    conv = conv.double()
    conv.load_state_dict(hc.perturb(sd0, c))
    mask = hc.coef_mask(c, ei.shape[1])
    F = ref_layers.F
    orig, used = F.dropout, []

    def dropout(t, p=0.5, training=True, inplace=False):
        if not training:
            return t
        used.append(1)
        return t * mask
    conv.train(c["train"])
    xr = x.clone().requires_grad_(True)
    F.dropout = dropout
    try:
        out = conv(xr, ei, w)
    finally:
        F.dropout = orig
    assert len(used) == (1 if c["train"] else 0), (name, used)
    (out * hc.cotangent(c, out.shape[0])).sum().backward()
    res = {f"{name}/chk": np.frombuffer(chk.encode(), dtype=np.uint8), f"{name}/keys": np.frombuffer("|".join(keys).encode(), dtype=np.uint8),
           f"{name}/out": out.detach().numpy(), f"{name}/grad_x": xr.grad.numpy()}
    for k, p in conv.named_parameters():
        res[f"{name}/grad:{k}"] = p.grad.numpy()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed fixture instead of writing it")
    a = ap.parse_args()
    ref_layers, _ = ref_shim.import_reference()
    ref_layers.HypergraphConv.propagate = _flow_propagate
    arrays = {}
    for name in sorted(hc.CASES):
        arrays.update(reference_case(name, ref_layers))
    path = os.path.join(ROOT, "tests", "golden", hc.FILE + ".npz")
    if a.check:
        tmp = path + ".check"
        hc.write_npz(tmp, arrays)
        try:
            same = open(tmp, "rb").read() == open(path, "rb").read()
        finally:
            os.remove(tmp)
        print("identical" if same else "DIFFERENT", path)
        sys.exit(0 if same else 1)
    hc.write_npz(path, arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
