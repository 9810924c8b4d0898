"""The cases of the HAN reference fixtures (tests/golden/baselines_han*.npz, written by tools/gen_han_fixtures.py): every input is
rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.  File format, checksum, sampling of large results
and the comparison helper are those of tests/baselines_cases.py.

A case's raw data is a list of (vertex, hyperedge) incidences: hyperedges of 2..8 members, two of one member, the last ``isolated``
vertex ids in no hyperedge, and five incidences listed twice (the metapath graphs binarise them away).  The metapath graphs come from
``dense_metapath_edges``, a dense numpy restatement.  Features are random on ALL n_v + n_e nodes (the driver's zero rows for hyperedge
nodes would put every pre-activation between two of them exactly on leaky_relu's kink).  No conv of any
case has a pre-activation within 1e-5 of the kink: the GPU comparison in fp32 asserts that margin from the float64 restatement
(tests/test_gpu_han.py), and tests/test_han_reference.py asserts it for every case here on the CPU."""
from __future__ import annotations

import numpy as np
import torch

from baselines_cases import WHOLE_MAX, assert_result, checksum, load, result, sample_idx, write_npz  # noqa: F401

# name: heads per layer (L = their number), training mode, sizes
CASES = {
    "han_h1_L1":       dict(heads=[1]),
    "han_h2_L1":       dict(heads=[2]),
    "han_h8_L1":       dict(heads=[8]),
    "han_h2_h2_L2":    dict(heads=[2, 2]),
    "han_h8_h1_L2":    dict(heads=[8, 1]),
    "han_h2_L1_train": dict(heads=[2], train=True),
    "han_h8_h2_train": dict(heads=[8, 2], train=True),
    # (one head: the Cora-shaped graphs have 75 000 edges, and with 8 heads there are so many pre-activations that some lie within 1e-5
    #  of the kink under every seed tried, 0..15; the head counts are covered by the small cases)
    "cora_han":        dict(heads=[1], n_v=2708, n_e=1579, F=1433, hidden=16, C=7, bow=True),
}
FILES = {"baselines_han": [k for k in CASES if not k.startswith("cora")], "baselines_han_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT = 0.6
KINK_MARGIN = 1e-5


def spec(name):
    c = dict(n_v=40, n_e=18, F=12, hidden=8, C=4, train=False, bow=False, isolated=3)
    c.update(CASES[name])
    c["seed"] = 5000 + sorted(CASES).index(name)
    return c


def raw_data(c):
    """(x float64 [n_v + n_e, F], incidences int64 [2, nnz] with zero-based hyperedge ids, n_v, n_e)."""
    rng = np.random.default_rng(c["seed"])
    n_v, n_e = c["n_v"], c["n_e"]
    used = n_v - c["isolated"]
    vs, es = [], []
    for e in range(n_e):
        k = 1 if e in (1, 5) else int(rng.integers(2, 9))
        mem = rng.choice(used, size=k, replace=False)
        vs += [int(v) for v in mem]
        es += [e] * k
    vs, es = vs + vs[:5], es + es[:5]                       # duplicate incidences
    n = n_v + n_e
    if c["bow"]:
        x = (rng.random((n, c["F"])) < 18.0 / c["F"]).astype(np.float64)
    else:
        x = rng.standard_normal((n, c["F"]))
    return x, np.stack([np.array(vs, dtype=np.int64), np.array(es, dtype=np.int64)]), n_v, n_e


def dense_metapath_edges(pairs, n_v, n_e):
    """[(row, col)] of VEV and EVE over n_v + n_e nodes from the dense incidence matrix: the non-zeros of the binarised H H^T on the
    vertex block / H^T H on the hyperedge block in row-major order, then one appended self-loop per node."""
    Hm = np.zeros((n_v, n_e))
    Hm[pairs[0], pairs[1]] = 1.0
    n = n_v + n_e
    out = []
    for A, base in ((Hm @ Hm.T, 0), (Hm.T @ Hm, n_v)):
        r, c = np.nonzero(A > 0)
        loops = np.arange(n, dtype=np.int64)
        out.append((np.concatenate([r + base, loops]).astype(np.int64), np.concatenate([c + base, loops]).astype(np.int64)))
    return out


def cotangent(c, n_rows):
    return np.random.default_rng(c["seed"] + 7).standard_normal((n_rows, c["C"]))


def masks(c, n_edges):
    """Explicit dropout factors of a training-mode case: ``masks[l][i] = (feat_keep [N, width of layer l's input], edge_keep
    [n_edges[i], heads of layer l])``; None in eval mode."""
    if not c["train"]:
        return None
    rng = np.random.default_rng(c["seed"] + 11)
    n = c["n_v"] + c["n_e"]
    draw = lambda *shape: (rng.random(shape) >= DROPOUT) / (1.0 - DROPOUT)
    out = []
    for l, H in enumerate(c["heads"]):
        width = c["F"] if l == 0 else c["hidden"] * c["heads"][l - 1]
        out.append([(draw(n, width), draw(E, H)) for E in n_edges])
    return out


def perturb(sd, c):
    """The fixture's parameters: the initial ones plus 0.1 * N(0, 1) (name order of the state_dict)."""
    rng = np.random.default_rng(c["seed"] + 3)
    return {k: v.detach().double() + 0.1 * torch.from_numpy(rng.standard_normal(tuple(v.shape))) for k, v in sd.items()}
