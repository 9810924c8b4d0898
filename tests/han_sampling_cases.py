"""The cases of the mini-batch HAN reference fixtures (tests/golden/baselines_han_sampling.npz, written by
tools/gen_han_sampling_fixtures.py): every input is rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.
File format, checksum, sampling of large results and the comparison helper are those of tests/baselines_cases.py; the raw incidences
are those of tests/han_cases.py (hyperedges of 2..8 members, two of one member, trailing isolated vertices, duplicate incidences).

A case's two blocks (VEV, EVE) are FIXED: built once per case by the numpy restatement of the sampler in tests/han_sampling_oracle.py
from the case's seed set -- ordinary vertices, the last isolated vertex and a hyperedge node in the small cases (so the VEV block has
self-loop-only targets and the EVE block has n_src > n_dst), 32 vertices with k = 20 in the Cora-shaped one.  Features are random on
all n_v + n_e nodes; a block's input is the rows of its source nodes.  No conv of any case has a pre-activation within 1e-5 of
leaky_relu's kink: the generator asserts it, and tests/test_han_sampling_reference.py asserts it from the restatement on the CPU."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np
import torch

import han_sampling_oracle as orc
from baselines_cases import WHOLE_MAX, assert_result, checksum, load, result, sample_idx, write_npz  # noqa: F401
from han_cases import perturb, raw_data  # noqa: F401

CASES = {
    "hs_h1":        dict(heads=[1]),
    "hs_h2":        dict(heads=[2]),
    "hs_h8":        dict(heads=[8]),
    "hs_h1_train":  dict(heads=[1], train=True),
    "hs_h2_train":  dict(heads=[2], train=True),
    "hs_h8_train":  dict(heads=[8], train=True),
    "cora_hs":      dict(heads=[8], n_v=2708, n_e=1579, F=1433, hidden=8, C=7, bow=True, B=32, k=20, mixed=False),
}
FILE = "baselines_han_sampling"
FILES = {FILE: list(CASES)}
DROPOUT = 0.6
KINK_MARGIN = 1e-5


def spec(name):
    c = dict(n_v=40, n_e=18, F=24, hidden=8, C=4, train=False, bow=False, isolated=3, B=10, k=5, mixed=True)
    c.update(CASES[name])
    c["seed"] = 7000 + sorted(CASES).index(name)
    return c


def seed_nodes(c):
    """The batch: distinct vertices that are in some hyperedge; in a ``mixed`` case the last two are replaced by the last isolated
    vertex and hyperedge node 3."""
    rng = np.random.default_rng(c["seed"] + 5)
    seeds = rng.choice(c["n_v"] - c["isolated"], size=c["B"], replace=False).astype(np.int64)
    if c["mixed"]:
        seeds[-2], seeds[-1] = c["n_v"] - 1, c["n_v"] + 3
    return seeds


def blocks(c, pairs=None):
    """``[VEV block, EVE block]``: SimpleNamespace(src_ids, src, dst int64 tensors; n_src, n_dst)."""
    if pairs is None:
        _, pairs, _, _ = raw_data(c)
    v2e, e2v = orc.adjacency(pairs, c["n_v"], c["n_e"])
    seeds = seed_nodes(c)
    out = []
    for mp in (0, 1):
        rng = np.random.default_rng(c["seed"] + 13 + mp)
        rows = orc.neighbour_rows(v2e, e2v, c["n_v"], mp, seeds, c["k"], rng)
        src_ids, src, dst, n_src, n_dst = orc.to_block(rows, seeds)
        out.append(SimpleNamespace(src_ids=torch.from_numpy(src_ids), src=torch.from_numpy(src), dst=torch.from_numpy(dst), n_src=n_src,
                                   n_dst=n_dst))
    return out


def cotangent(c):
    return np.random.default_rng(c["seed"] + 7).standard_normal((c["B"], c["C"]))


def masks(c, blks):
    """Explicit dropout factors of a training-mode case: ``masks[i] = (feat_keep [n_src_i, F], edge_keep [nnz_i, heads])``."""
    if not c["train"]:
        return None
    rng = np.random.default_rng(c["seed"] + 11)
    draw = lambda *shape: (rng.random(shape) >= DROPOUT) / (1.0 - DROPOUT)
    return [(draw(b.n_src, c["F"]), draw(b.src.numel(), c["heads"][0])) for b in blks]
