"""The cases of the CEGCN reference fixtures (tests/golden/baselines_ce_*.npz, written by tools/gen_ce_fixtures.py): every input is
rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.  File format, checksum, sampling of large
results and the comparison helper are those of tests/baselines_cases.py.

A case's raw data is the loaders' block edge list ``[[V | E], [E | V]]``.  Hyperedges have 2..8 members, a few have one (they add
no pair), the first two vertices share three more hyperedges (a pair of multiplicity >= 3), the ``interior`` vertex ids and the
last ``trailing`` ids are in no hyperedge (an interior one gets a GCN self-loop, a trailing one none: its output is the bias)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

from baselines_cases import WHOLE_MAX, assert_result, checksum, load, result, sample_idx, write_npz  # noqa: F401

# name: layers, normalisation, training mode, sizes
CASES = {
    "cegcn_L1":          dict(L=1, norm="ln"),
    "cegcn_L2":          dict(L=2, norm="ln"),
    "cegcn_L3":          dict(L=3, norm="ln"),
    "cegcn_L2_bn":       dict(L=2, norm="bn"),
    "cegcn_L3_bn_train": dict(L=3, norm="bn", train=True),
    "cegcn_L2_train":    dict(L=2, norm="ln", train=True),
    "cora_cegcn":        dict(L=2, norm="ln", n_v=2708, n_e=1579, F=1433, hidden=64, C=7, bow=True, interior=(), trailing=3),
}
FILES = {"baselines_ce": [k for k in CASES if not k.startswith("cora")],
         "baselines_ce_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT = 0.5


def spec(name):
    c = dict(n_v=60, n_e=25, F=12, hidden=16, C=4, train=False, bow=False, interior=(7, 30), trailing=4)
    c.update(CASES[name])
    c["seed"] = 2000 + sorted(CASES).index(name)
    return c


def args_of(c):
    return SimpleNamespace(method="CEGCN", All_num_layers=c["L"], dropout=DROPOUT, MLP_hidden=c["hidden"], num_features=c["F"],
                           num_classes=c["C"], normalization=c["norm"])


def raw_data(c):
    """(x float64 [n_v, F], block edge list int64, n_v, n_e)."""
    rng = np.random.default_rng(c["seed"])
    n_v, n_e = c["n_v"], c["n_e"]
    pool = np.array([v for v in range(n_v - c["trailing"]) if v not in c["interior"]])
    nodes, hes = [], []
    for e in range(n_e):
        if e >= n_e - 3:
            mem = pool[:2]                                  # the shared pair, in the last three hyperedges
        else:
            k = 1 if e % 9 == 1 else int(rng.integers(2, 9))
            mem = rng.choice(pool, size=k, replace=False)
        nodes += [int(v) for v in mem]
        hes += [e] * len(mem)
    v = np.array(nodes, dtype=np.int64)
    e = np.array(hes, dtype=np.int64) + n_v
    ei = np.concatenate([np.stack([v, e]), np.stack([e, v])], axis=1)
    span = int(ei.max()) + 1
    key = np.unique(ei[0] * span + ei[1])
    block = np.stack([key // span, key % span])
    if c["bow"]:
        x = (rng.random((n_v, c["F"])) < 18.0 / c["F"]).astype(np.float64)
    else:
        x = rng.standard_normal((n_v, c["F"]))
    return x, block, n_v, n_e


def cotangent(c, n_rows):
    return np.random.default_rng(c["seed"] + 7).standard_normal((n_rows, c["C"]))


def masks(c):
    """Explicit dropout factors, one [n_v, hidden] array per dropout site (between convs) of a training-mode case."""
    if not c["train"]:
        return []
    rng = np.random.default_rng(c["seed"] + 11)
    return [(rng.random((c["n_v"], c["hidden"])) >= DROPOUT) / (1.0 - DROPOUT) for _ in range(max(c["L"], 2) - 1)]


def perturb(sd, c):
    """The fixture's parameters: the initial floating-point entries plus 0.1 * N(0, 1) (name order; the BatchNorm running variance
    plus 0.1 * |N(0, 1)|), integer entries as they are."""
    rng = np.random.default_rng(c["seed"] + 3)
    out = {}
    for k, v in sd.items():
        if not v.is_floating_point():
            out[k] = v.clone()
            continue
        z = torch.from_numpy(rng.standard_normal(tuple(v.shape)))
        out[k] = v.detach().double() + 0.1 * (z.abs() if k.endswith("running_var") else z)
    return out
