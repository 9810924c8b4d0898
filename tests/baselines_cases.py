"""The cases of the HGNN / HCHA / HNHN reference fixtures (tests/golden/baselines_*.npz, written by tools/gen_baseline_fixtures.py):
every input is rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.

A case's raw data is the reference loaders' block edge list ``[[V | E], [E | V]]`` (hyperedge ids behind the vertex ids), which
``train.preprocess`` and the reference's preprocessing branch (train.py:375-388) both start from.  Parameters are the model's initial
ones under ``torch.manual_seed(seed)`` (the fixture records the reference's checksum of them) plus a seeded perturbation, so that
HCHA's zero-initialised biases are not zero."""
from __future__ import annotations

import hashlib
import io
import os
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SAMPLE = 256                 # entries kept of a result with more than WHOLE_MAX entries (plus its sum and absolute sum)
WHOLE_MAX = 20000

# name: method, layers, symdegnorm, nonlinear_inbetween, self-loops, interior empty hyperedge, isolated vertices, sizes, training
CASES = {
    "hcha_L2":        dict(method="HCHA", L=2, sym=False, self_loops=True, n_v=60, n_e=25, F=12),
    "hcha_L3":        dict(method="HCHA", L=3, sym=False, self_loops=True, n_v=60, n_e=25, F=12),
    "hcha_L2_train":  dict(method="HCHA", L=2, sym=False, self_loops=True, n_v=60, n_e=25, F=12, train=True),
    "hcha_empty":     dict(method="HCHA", L=2, sym=False, self_loops=True, n_v=60, n_e=25, F=12, empty=True),
    "hcha_noself":    dict(method="HCHA", L=2, sym=False, self_loops=False, n_v=60, n_e=25, F=12, isolated=4),
    "hgnn_L2":        dict(method="HGNN", L=2, sym=True, self_loops=True, n_v=60, n_e=25, F=12),
    "hgnn_L3_train":  dict(method="HGNN", L=3, sym=True, self_loops=True, n_v=60, n_e=25, F=12, train=True),
    "hgnn_noself":    dict(method="HGNN", L=2, sym=True, self_loops=False, n_v=60, n_e=25, F=12, isolated=4, empty=True),
    "hnhn_L1":        dict(method="HNHN", L=1, self_loops=True, n_v=60, n_e=25, F=12),
    "hnhn_L2":        dict(method="HNHN", L=2, self_loops=True, n_v=60, n_e=25, F=12),
    "hnhn_L2_linear": dict(method="HNHN", L=2, self_loops=True, n_v=60, n_e=25, F=12, nonlinear=False),
    "hnhn_L2_train":  dict(method="HNHN", L=2, self_loops=True, n_v=60, n_e=25, F=12, train=True),
    "hnhn_noself":    dict(method="HNHN", L=2, self_loops=False, n_v=60, n_e=25, F=12, isolated=4),
    "cora_hcha":      dict(method="HCHA", L=2, sym=False, self_loops=True, n_v=2708, n_e=1579, F=1433, hidden=64, C=7, bow=True),
    "cora_hnhn":      dict(method="HNHN", L=2, self_loops=True, n_v=2708, n_e=1579, F=1433, hidden=64, C=7, bow=True),
}
FILES = {"baselines_hcha": [k for k in CASES if k.startswith(("hcha", "hgnn"))],
         "baselines_hnhn": [k for k in CASES if k.startswith("hnhn")],
         "baselines_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT = 0.5


def spec(name):
    c = dict(sym=False, nonlinear=True, empty=False, isolated=0, hidden=16, C=4, train=False, bow=False)
    c.update(CASES[name])
    c["seed"] = 1000 + sorted(CASES).index(name)
    return c


def args_of(c):
    return SimpleNamespace(method=c["method"], All_num_layers=c["L"], dropout=DROPOUT, MLP_hidden=c["hidden"], num_features=c["F"],
                           num_classes=c["C"], HCHA_symdegnorm=c["sym"], HNHN_alpha=-1.5, HNHN_beta=-0.5,
                           HNHN_nonlinear_inbetween=c["nonlinear"], add_self_loop=c["self_loops"])


def raw_data(c):
    """(x float64 [n_v, F], block edge list int64, n_v, n_e).  Hyperedge sizes 1..8 (one of a single member), the last hyperedge
    never empty (the reference's ExtractV2E checks the largest id), optionally one empty interior hyperedge and ``isolated``
    trailing vertices in no hyperedge."""
    rng = np.random.default_rng(c["seed"])
    n_v, n_e = c["n_v"], c["n_e"]
    used = n_v - c["isolated"]
    nodes, hes = [], []
    for e in range(n_e):
        if c["empty"] and e == n_e // 2:
            continue
        k = 1 if e == 1 else int(rng.integers(2, 9))
        mem = rng.choice(used, size=min(k, used), replace=False)
        nodes += [int(v) for v in mem]
        hes += [e] * len(mem)
    v = np.array(nodes, dtype=np.int64)
    e = np.array(hes, dtype=np.int64) + n_v
    ei = np.concatenate([np.stack([v, e]), np.stack([e, v])], axis=1)
    span = int(ei.max()) + 1
    key = np.unique(ei[0] * span + ei[1])
    block = np.stack([key // span, key % span])
    if c["bow"]:                                            # binary bag-of-words rows, ~18 words each
        x = (rng.random((n_v, c["F"])) < 18.0 / c["F"]).astype(np.float64)
    else:
        x = rng.standard_normal((n_v, c["F"]))
    return x, block, n_v, n_e


def cotangent(c, n_rows):
    return np.random.default_rng(c["seed"] + 7).standard_normal((n_rows, c["C"]))


def masks(c):
    """Explicit dropout factors (0 or 1 / (1 - p)), one [n_v, hidden] array per dropout site of a training-mode case."""
    if not c["train"]:
        return []
    n_sites = (max(c["L"], 2) if c["method"] != "HNHN" else c["L"]) - 1
    rng = np.random.default_rng(c["seed"] + 11)
    return [(rng.random((c["n_v"], c["hidden"])) >= DROPOUT) / (1.0 - DROPOUT) for _ in range(n_sites)]


def perturb(sd, c):
    """The fixture's parameters: the initial ones plus 0.1 * N(0, 1) (name order of the state_dict)."""
    rng = np.random.default_rng(c["seed"] + 3)
    return {k: v.detach().double() + 0.1 * torch.from_numpy(rng.standard_normal(tuple(v.shape))) for k, v in sd.items()}


def checksum(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(str(tuple(v.shape)).encode())
        h.update(str(v.dtype).encode())
        h.update(np.ascontiguousarray(v.detach().cpu().numpy()).tobytes())
    return h.hexdigest()


def sample_idx(key: str, size: int) -> np.ndarray:
    rng = np.random.default_rng(int(hashlib.sha256(key.encode()).hexdigest()[:8], 16))
    return np.sort(rng.choice(size, size=SAMPLE, replace=False))


# ---- the fixture files: a zip of .npy members with fixed timestamps (regenerates byte for byte) ---------------------------------
def write_npz(path: str, arrays: dict) -> None:
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def load(file: str) -> dict:
    with np.load(os.path.join(GOLDEN, file + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def result(fx: dict, case: str, key: str):
    """A recorded result: ('whole', array) or ('sample', (flat indices, values, sum, abs-sum, shape))."""
    p = f"{case}/{key}"
    if p in fx:
        return "whole", fx[p]
    return "sample", (fx[p + ":idx"], fx[p + ":val"], float(fx[p + ":sum"]), float(fx[p + ":abs"]), tuple(fx[p + ":shape"]))


def assert_result(got: torch.Tensor, fx: dict, case: str, key: str, rtol: float, atol: float, equal_nan: bool = False):
    kind, v = result(fx, case, key)
    got = got.detach().cpu().double()
    if kind == "whole":
        torch.testing.assert_close(got, torch.from_numpy(v).reshape(got.shape), rtol=rtol, atol=atol, equal_nan=equal_nan,
                                   msg=lambda m: f"{case}/{key}: {m}")
        return
    idx, val, s, a, shape = v
    assert tuple(got.shape) == shape, (case, key, tuple(got.shape), shape)
    flat = got.reshape(-1)
    torch.testing.assert_close(flat[torch.from_numpy(idx)], torch.from_numpy(val), rtol=rtol, atol=atol, equal_nan=equal_nan,
                               msg=lambda m: f"{case}/{key} (sampled): {m}")
    if not (equal_nan and np.isnan(s)):
        bound = rtol * a + atol * flat.numel()
        assert abs(float(flat.sum()) - s) <= bound, (case, key, "sum", float(flat.sum()), s, bound)
        assert abs(float(flat.abs().sum()) - a) <= bound, (case, key, "abs-sum", float(flat.abs().sum()), a, bound)
