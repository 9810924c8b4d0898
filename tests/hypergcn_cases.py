"""The cases of the HyperGCN reference fixtures (tests/golden/baselines_hypergcn*.npz, written by tools/gen_hypergcn_fixtures.py): every
input is rebuilt here from fixed seeds, so the fixtures hold only what the reference computed (and the numpy projection vectors it
drew).  File format, checksum, sampling of large results and the comparison helper are those of tests/baselines_cases.py.

A case's hypergraph is a list of (vertex, hyperedge) pairs with hyperedge ids from 0, sorted by vertex as ``ExtractV2E`` leaves them
(``shuffle``: in a seeded random order instead, so that "first in edge-list order" is not "smallest vertex id"): hyperedges of 2..8
members, hyperedge 0 of two (c = 1) and hyperedge 1 of three (c = 3), hyperedges 5..7 one shared member set, ``singletons`` two
hyperedges of one member (cases without mediators only), the vertices of ``interior`` and the last ``trailing`` ids in no hyperedge
(D = 1).  ``ties``: vertices 0 and 1 get all-zero feature rows and share hyperedge 3 whose other members have strictly positive rows
(a joint arg-min: the projection of a zero row is exactly 0 in any arithmetic), and the three members of hyperedge 4 are zero rows
too (S = I with k = 3).  Tie cases are fast mode only: there Z is the input and equal rows give bit-equal projections."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from baselines_cases import WHOLE_MAX, assert_result, checksum, load, perturb, result, sample_idx, write_npz  # noqa: F401

# name: layers, fast, mediators, training mode, sizes.  ``reseed`` moves a case to another seed where the first one misses
# RELU_MARGIN or GAP_MARGIN on the float64 restatement (found on the CPU with the restatement alone;
# tests/test_hypergcn_reference.py asserts both for every case).
CASES = {
    "hg_L1_fast_med":         dict(L=1, fast=True, med=True),
    "hg_L2_fast_med":         dict(L=2, fast=True, med=True),
    "hg_L2_fast_nomed":       dict(L=2, fast=True, med=False, singletons=True),
    "hg_L2_slow_med":         dict(L=2, fast=False, med=True),
    "hg_L2_slow_nomed":       dict(L=2, fast=False, med=False, singletons=True),
    "hg_L3_slow_med_train":   dict(L=3, fast=False, med=True, train=True),
    "hg_L2_fast_med_train":   dict(L=2, fast=True, med=True, train=True),
    "hg_L2_slow_nomed_train": dict(L=2, fast=False, med=False, singletons=True, train=True),
    "hg_L3_citeseer":         dict(L=3, fast=True, med=True, dname="citeseer"),
    "hg_ties_fast_med":       dict(L=2, fast=True, med=True, ties=True, shuffle=True),
    "hg_ties_fast_nomed":     dict(L=2, fast=True, med=False, ties=True, shuffle=True, singletons=True),
    # Cora-shaped: 2708 x 1433 binary bag-of-words rows, 1579 hyperedges.  Fast mode only (see GAP_MARGIN below).
    "cora_hypergcn_fast":     dict(L=2, fast=True, med=True, n_v=2708, n_e=1579, F=1433, C=7, bow=True, interior=(), trailing=0),
}
FILES = {"baselines_hypergcn": [k for k in CASES if not k.startswith("cora")],
         "baselines_hypergcn_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT = 0.5
RELU_MARGIN = 1e-6           # smallest |pre-activation| / (largest of its row): an order above the rounding of fp32 sums (unigcnii_cases)

# GAP_MARGIN: the smallest admissible (extreme - runner-up) gap of a hyperedge's projections, at both ends, relative to
# max_i sum_j |Z[m_i, j]| rv_j.  The product computes p_i = sum_j Z[m_i, j] rv_j in fp32: the running-error bound of a dot of n
# non-zero terms is n * u * sum_j |Z_ij| rv_j with u = 2^-24.  In the re-approximating mode Z = H W is itself an fp32 GEMM of inner
# dimension K whose entries carry up to K * u of their own absolute sums, which adds K roundings on the same scale.  So the order of
# two projections can differ between the product and the float64 reference only where their gap is within (n + K) * u of that scale;
# an order of magnitude on top gives the margin.  GAP_TERMS = 64 covers every case here: the small cases have n <= 32 output columns
# and K <= 32 input columns in the re-approximating mode (widths 12 -> 32 -> 16 -> 4) and n = F = 12 in fast mode; the Cora-shaped
# bag-of-words rows hold at most 64 non-zeros (asserted in tests/test_hypergcn_reference.py), K = 0 in fast mode.
# The Cora shape is FAST-ONLY: its re-approximating first layer has K = 1433, n = 16, a margin of 10 * 1449 * 2^-24 = 8.6e-4, and with
# 1579 hyperedges x 2 ends each of the four seeds tried (the float64 restatement alone, on the CPU) leaves 8 to 12 gaps per layer
# below that, the smallest between 1e-5 and 2e-4 -- so the shape runs in fast mode only, where it clears GAP_MARGIN.
GAP_TERMS = 64
GAP_MARGIN = 10 * GAP_TERMS * 2.0 ** -24


def spec(name):
    c = dict(n_v=60, n_e=25, F=12, C=4, train=False, bow=False, ties=False, shuffle=False, singletons=False, dname="synthetic",
             interior=(7, 30), trailing=4)
    c.update(CASES[name])
    c["seed"] = 7000 + sorted(CASES).index(name) + 100 * c.pop("reseed", 0)
    return c


def widths(c):
    """[F, 2^(L+2), ..., 2^4, C]; exponents two higher for citeseer (reference models.py:40-46)."""
    L = c["L"]
    return [c["F"]] + [2 ** (L - i + (4 if c["dname"] == "citeseer" else 2)) for i in range(L - 1)] + [c["C"]]


def args_of(c):
    return SimpleNamespace(method="HyperGCN", All_num_layers=c["L"], dropout=DROPOUT, num_features=c["F"], num_classes=c["C"],
                           HyperGCN_mediators=c["med"], HyperGCN_fast=c["fast"], dname=c["dname"], cuda=0)


def raw_data(c):
    """(x float64 [n_v, F], pairs int64 [2, nnz]: row 0 vertex ids, row 1 hyperedge ids from 0, n_v, n_e)."""
    rng = np.random.default_rng(c["seed"])
    n_v, n_e = c["n_v"], c["n_e"]
    free = [v for v in range(n_v - c["trailing"]) if v not in c["interior"]]
    if c["bow"]:
        x = (rng.random((n_v, c["F"])) < 18.0 / c["F"]).astype(np.float64)
        x[np.arange(n_v), rng.integers(0, c["F"], n_v)] = 1.0                  # no empty row
    else:
        x = rng.standard_normal((n_v, c["F"]))
    members = []
    for e in range(n_e):
        k = 2 if e == 0 else 3 if e == 1 else int(rng.integers(2, 9))
        if c["singletons"] and e in (2, n_e - 2):
            k = 1
        members.append([int(v) for v in rng.choice(free, size=k, replace=False)])
    members[6] = list(members[5])
    members[7] = list(members[5])
    if c["ties"]:
        others = [v for v in free if v > 4][:3]
        members[3] = [others[0], 1, others[1], 0, others[2]]
        members[4] = [2, 3, 4]
        x[:5] = 0.0
        x[others] = np.abs(x[others]) + 0.5
    v = np.array([m for mem in members for m in mem], dtype=np.int64)
    e = np.array([i for i, mem in enumerate(members) for _ in mem], dtype=np.int64)
    order = rng.permutation(v.size) if c["shuffle"] else np.lexsort((e, v))
    return x, np.stack([v[order], e[order]]), n_v, n_e


def member_lists(pairs, n_e):
    """hyperedge -> members in the order the pairs list them (the reference's ``He_dict`` values)."""
    out = [[] for _ in range(n_e)]
    for v, e in zip(pairs[0].tolist(), pairs[1].tolist()):
        out[e].append(v)
    return out


def rv_sizes(c):
    """Lengths of the projection vectors the reference draws, in order: one [F] at construction (fast), else one per layer output."""
    h = widths(c)
    return [h[0]] if c["fast"] else h[1:]


def cotangent(c, n_rows):
    return np.random.default_rng(c["seed"] + 7).standard_normal((n_rows, c["C"]))


def masks(c):
    """Explicit dropout factors of a training-mode case: one [n_v, width] per layer but the last."""
    if not c["train"]:
        return []
    rng = np.random.default_rng(c["seed"] + 11)
    return [(rng.random((c["n_v"], w)) >= DROPOUT) / (1.0 - DROPOUT) for w in widths(c)[1:-1]]
