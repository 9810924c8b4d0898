"""The cases of the heterogeneous-HAN reference fixtures (tests/golden/baselines_han_hetero.npz, written by
tools/gen_han_hetero_fixtures.py).  Every input is rebuilt here from fixed seeds; the fixtures also record the inputs, so a drift of
this file shows.  File format, checksum and comparison helper are those of tests/baselines_cases.py.

A case is an ACM-shaped typed graph: papers, authors, fields with the relations pa / ap / pf / fp; every paper has one field, most
papers have 1..3 authors, the ``orphans`` last paper ids have none (PAP rows without an incoming edge), four pa pairs are listed
twice.  Features are random normal rows on the papers.  No conv of any case has a pre-activation within 1e-5 of leaky_relu's kink --
the criterion of tests/han_cases.py, asserted on the CPU by tests/test_han_hetero_reference.py."""
from __future__ import annotations

import numpy as np
import torch

from baselines_cases import assert_result, checksum, load, write_npz  # noqa: F401
from han_cases import DROPOUT, KINK_MARGIN  # noqa: F401

META_PATHS = [["pa", "ap"], ["pf", "fp"]]
CASES = {
    "hetero_h1":       dict(heads=[1]),
    "hetero_h4_h2":    dict(heads=[4, 2], bump=1),      # (bump 0 leaves one pre-activation 7.5e-6 from the kink: the first that clears 1e-5)
    "hetero_h2_train": dict(heads=[2], train=True),
}
FILE = "baselines_han_hetero"
RELATIONS = [("paper", "pa", "author"), ("author", "ap", "paper"), ("paper", "pf", "field"), ("field", "fp", "paper")]


def spec(name):
    c = dict(n_p=40, n_a=25, n_f=4, F=12, hidden=8, C=3, train=False, orphans=4, bump=0)
    c.update(CASES[name])
    c["seed"] = 7000 + sorted(CASES).index(name) + 10 * c["bump"]
    return c


def raw_data(c):
    """``(x float64 [n_p, F], edges {relation: (src, dst) int64 numpy}, num_nodes)``."""
    rng = np.random.default_rng(c["seed"])
    n_p, n_a, n_f = c["n_p"], c["n_a"], c["n_f"]
    ps, as_ = [], []
    for p in range(n_p - c["orphans"]):
        k = int(rng.integers(1, 4))
        mem = rng.choice(n_a - 2, size=k, replace=False)               # (the last two authors have no paper)
        ps += [p] * k
        as_ += [int(a) for a in mem]
    ps, as_ = ps + ps[:4], as_ + as_[:4]                               # duplicate pairs
    pa = (np.array(ps, dtype=np.int64), np.array(as_, dtype=np.int64))
    field = np.minimum(rng.geometric(0.55, size=n_p) - 1, n_f - 1).astype(np.int64)      # skewed field sizes
    papers = np.arange(n_p, dtype=np.int64)
    edges = {RELATIONS[0]: pa, RELATIONS[1]: (pa[1], pa[0]), RELATIONS[2]: (papers, field), RELATIONS[3]: (field, papers)}
    return rng.standard_normal((n_p, c["F"])), edges, {"paper": n_p, "author": n_a, "field": n_f}


def cotangent(c, n_rows):
    return np.random.default_rng(c["seed"] + 7).standard_normal((n_rows, c["C"]))


def masks(c, n_edges):
    """Explicit dropout factors of a training-mode case, as tests/han_cases.py draws them; None in eval mode."""
    if not c["train"]:
        return None
    rng = np.random.default_rng(c["seed"] + 11)
    draw = lambda *shape: (rng.random(shape) >= DROPOUT) / (1.0 - DROPOUT)
    out = []
    for l, H in enumerate(c["heads"]):
        width = c["F"] if l == 0 else c["hidden"] * c["heads"][l - 1]
        out.append([(draw(c["n_p"], width), draw(E, H)) for E in n_edges])
    return out


def perturb(sd, c):
    """The fixture's parameters: the initial ones plus 0.1 * N(0, 1) (name order of the state_dict); the conv biases become non-zero,
    so an empty row's elu(bias) is not 0."""
    rng = np.random.default_rng(c["seed"] + 3)
    return {k: v.detach().double() + 0.1 * torch.from_numpy(rng.standard_normal(tuple(v.shape))) for k, v in sd.items()}
