"""Seeded inputs of the hypergraph-attention tests and the cases of the reference fixture tests/golden/baselines_hcha_attn.npz
(written by tools/gen_hcha_attn_fixtures.py): every input is rebuilt here from fixed seeds, so the fixture holds only what the
reference's ``HypergraphConv(use_attention=True)`` computed.

A fixture case is one conv on ``n_v = 60`` vertices and ``n_e = 25`` hyperedges of 1..8 members WITHOUT self-loop hyperedges (the
reference indexes vertex rows by hyperedge id, so it needs n_e <= n_v), 12 input channels.  Parameters: the layer's initial ones
under ``torch.manual_seed(seed)`` (the fixture records the reference's checksum of them) plus a seeded perturbation, so that the
zero-initialised bias is not zero."""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from baselines_cases import checksum, load, write_npz  # noqa: E402,F401

FILE = "baselines_hcha_attn"
N_V, N_E, F_IN = 60, 25, 12
ATTN_DROP = 0.5

# name: heads, out channels, concat; empty interior hyperedge, isolated trailing vertices, hyperedge weights, training mode
CASES = {
    "h1_concat":        dict(heads=1, out=16, concat=True),
    "h4_concat":        dict(heads=4, out=8, concat=True),
    "h3_mean":          dict(heads=3, out=5, concat=False),
    "h4_empty":         dict(heads=4, out=8, concat=True, empty=True),
    "h3_mean_isolated": dict(heads=3, out=5, concat=False, isolated=4),
    "h1_weight":        dict(heads=1, out=16, concat=True, weight=True),
    "h4_weight_mean":   dict(heads=4, out=8, concat=False, weight=True, empty=True),
    "h4_train":         dict(heads=4, out=8, concat=True, train=True),
}


def spec(name):
    c = dict(empty=False, isolated=0, weight=False, train=False)
    c.update(CASES[name])
    c["seed"] = 2000 + sorted(CASES).index(name)
    return c


def hypergraph(n_v, n_e, seed, empty=True, isolated=0, dup=False, hub=False, long_row=0):
    """[2, nnz] int64 (vertex, hyperedge) pairs: random sizes 1..8, hyperedge 1 a singleton, the last hyperedge never empty,
    optionally an empty interior hyperedge, ``isolated`` trailing vertices without incidences, a duplicated incidence, vertex 0 in
    every hyperedge (``hub``: one long vertex-major row) and hyperedge 0 with ``long_row`` members."""
    rng = np.random.default_rng(seed)
    used = n_v - isolated
    pairs = []
    for e in range(n_e):
        if empty and e == n_e // 2:
            continue
        k = 1 if e == 1 else int(rng.integers(1, 9))
        mem = [int(v) for v in rng.choice(np.arange(1 if hub else 0, used), size=min(k, used - 1), replace=False)]
        if hub:
            mem.append(0)
        pairs += [(v, e) for v in mem]
    if long_row:
        have = {v for v, e in pairs if e == 0}
        extra = [int(v) for v in rng.choice(used, size=min(long_row, used), replace=False) if int(v) not in have]
        pairs += [(v, 0) for v in extra]
    if dup:
        pairs.append(pairs[3])
    return torch.tensor(pairs, dtype=torch.int64).t().contiguous()


def inputs(c):
    """(x float64 [n_v, F_in], edge list int64 [2, nnz], hyperedge weights float64 [n_e] or None)."""
    rng = np.random.default_rng(c["seed"])
    ei = hypergraph(N_V, N_E, c["seed"], empty=c["empty"], isolated=c["isolated"])
    x = torch.from_numpy(rng.standard_normal((N_V, F_IN)))
    w = torch.from_numpy(rng.uniform(0.5, 1.5, size=N_E)) if c["weight"] else None
    return x, ei, w


def cotangent(c, n_rows):
    width = c["heads"] * c["out"] if c["concat"] else c["out"]
    return torch.from_numpy(np.random.default_rng(c["seed"] + 7).standard_normal((n_rows, width)))


def coef_mask(c, nnz):
    """The explicit factor (0 or 1 / (1 - p)) that replaces ``F.dropout`` on the [nnz, heads] coefficients of a training-mode case."""
    if not c["train"]:
        return None
    rng = np.random.default_rng(c["seed"] + 11)
    return torch.from_numpy((rng.random((nnz, c["heads"])) >= ATTN_DROP) / (1.0 - ATTN_DROP))


def perturb(sd, c):
    """The fixture's parameters: the initial ones plus 0.1 * N(0, 1) (name order of the state_dict)."""
    rng = np.random.default_rng(c["seed"] + 3)
    return {k: v.detach().double() + 0.1 * torch.from_numpy(rng.standard_normal(tuple(v.shape))) for k, v in sd.items()}
