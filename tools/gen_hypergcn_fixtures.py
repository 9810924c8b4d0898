"""Record the REFERENCE's HyperGCN (reference models.py:29-77, utils.py:11-243) on the cases of tests/hypergcn_cases.py into
tests/golden/baselines_hypergcn*.npz.  Container-only: imports the reference's models (and through them its utils) via
oracle/ref_shim.py (read-only).  Regenerates byte for byte: ``python tools/gen_hypergcn_fixtures.py`` (``--check``: compare with the
committed files instead of writing).

The reference runs as it is written -- float32 parameters and activations, the Laplacian through numpy float64 projections, a Python
dict, scipy float32 and a torch sparse tensor -- on the CPU: each layer's hard-coded ``cuda:N`` ``device`` attribute is assigned the
CPU device.  ``np.random.seed(case seed)`` fixes the projection vectors; they are re-drawn here in the same order and recorded
(``rv0``, ``rv1``, ...).  ``utils.Laplacian`` is wrapped at run time to keep every adjacency it returns, and ``models.F`` is replaced
for the run by a namespace whose ``dropout`` multiplies with the case's explicit factors in call order.

What each case records: the projection vectors; every coalesced ``A`` (indices + values; for a matrix with more than WHOLE_MAX / 2
entries its product with a seeded probe instead); the checksum and layout of the initial ``state_dict`` under ``torch.manual_seed``;
with the case's perturbed parameters: logits, d(sum(logits * G))/dx and every parameter gradient.

The process pins its arithmetic (see the environment block below the imports) so that the files regenerate byte for byte on any
x86-64 CPU, whatever its vector extensions and core count."""
from __future__ import annotations

import argparse
import os
import sys
from types import SimpleNamespace

# The recorded float32 results must not depend on the vector extensions or the core count of the CPU that regenerates them: MKL's
# SSE2-only "compatible" code path (conditional numerical reproducibility), ATen's AVX2 kernels rather than wider ones (not its
# baseline kernels: their ``uniform_`` stream differs, and the recorded checksum of the initial draw is compared with a draw
# made by an ordinary process), one thread.  Set before numpy and torch load their libraries.
os.environ.update(MKL_CBWR="COMPATIBLE", ATEN_CPU_CAPABILITY="avx2", OMP_NUM_THREADS="1", MKL_NUM_THREADS="1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(1)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import hypergcn_cases as hc  # noqa: E402
from gen_ce_fixtures import _put  # noqa: E402
from oracle import ref_shim  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def probe(n):
    return np.random.default_rng(n).standard_normal((n, 3))


def reference_case(name, ref_models):
    ref_utils = ref_models.utils
    c = hc.spec(name)
    x, pairs, n_v, n_e = hc.raw_data(c)
    He = {e: mem for e, mem in enumerate(hc.member_lists(pairs, n_e)) if mem}
    args = hc.args_of(c)
    xt = torch.from_numpy(x).float()
    kept = []
    real_lap, real_F = ref_utils.Laplacian, ref_models.F

    def lap(*a):
        A = real_lap(*a)
        kept.append(A.coalesce())
        return A

    masks = [torch.from_numpy(m).float() for m in hc.masks(c)]
    used = []

    def dropout(t, p, training=True):
        if not training:
            return t
        used.append(1)
        return t * masks[len(used) - 1]

    ref_utils.Laplacian = lap
    ref_models.F = SimpleNamespace(relu=torch.nn.functional.relu, dropout=dropout)
    try:
        np.random.seed(c["seed"])
        torch.manual_seed(c["seed"])
        model = ref_models.HyperGCN(n_v, He, xt.numpy(), c["F"], c["L"], c["C"], args)
        for layer in model.layers:
            layer.device = torch.device("cpu")
        chk = hc.checksum(model.state_dict())
        spec = [(k, tuple(v.shape), str(v.dtype)) for k, v in model.state_dict().items()]
        model.load_state_dict({k: v.float() for k, v in hc.perturb(model.state_dict(), c).items()})
        xr = xt.clone().requires_grad_(True)
        model.train(c["train"])
        logits = model(SimpleNamespace(x=xr))
        assert len(used) == len(masks), (name, len(used), len(masks))
        G = torch.from_numpy(hc.cotangent(c, logits.shape[0])).float()
        (logits * G).sum().backward()
    finally:
        ref_utils.Laplacian, ref_models.F = real_lap, real_F
    np.random.seed(c["seed"])                                     # the same stream again: what Laplacian drew, in order
    rvs = [np.random.rand(k) for k in hc.rv_sizes(c)]
    assert len(kept) == len(rvs), (name, len(kept), len(rvs))
    # (float32 results stored as float64: the comparison helper of tests/baselines_cases.py compares in that type)
    return dict(rvs=rvs, A=kept, chk=chk, spec=spec, logits=logits.detach().double(), grad_x=xr.grad.detach().double(),
                grads={k: p.grad.detach().double() for k, p in model.named_parameters()})


def build(file, ref_models) -> dict:
    arrays = {}
    for name in hc.FILES[file]:
        r = reference_case(name, ref_models)
        for i, rv in enumerate(r["rvs"]):
            arrays[f"{name}/rv{i}"] = rv
        for i, A in enumerate(r["A"]):
            if A._nnz() <= hc.WHOLE_MAX // 2:
                arrays[f"{name}/A{i}:indices"] = A.indices().numpy().astype(np.int32)
                arrays[f"{name}/A{i}:values"] = A.values().numpy()
            else:
                arrays[f"{name}/A{i}:nnz"] = np.int64(A._nnz())
                arrays[f"{name}/A{i}:matvec"] = torch.sparse.mm(A.double(), torch.from_numpy(probe(A.shape[0]))).numpy()
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
    _, ref_models = ref_shim.import_reference()
    for file in hc.FILES:
        arrays = build(file, ref_models)
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


if __name__ == "__main__":
    main()
