"""The cases of the UniGCNII reference fixtures (tests/golden/baselines_unigcnii*.npz, written by tools/gen_unigcnii_fixtures.py): every
input is rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.  Raw data, file format, checksum,
sampling of large results and the comparison helper are those of tests/ce_cases.py / tests/baselines_cases.py: hyperedges of 2..8
members, a few of one, a member set shared by three hyperedges, ``interior`` and the last ``trailing`` vertex ids in no hyperedge.
With ``self_loops`` (the driver's default) every vertex gets a singleton hyperedge; without, the isolated vertices keep a zero row
of the incidence matrix (degV: inf -> 1; under ``use_norm`` a zero row norm) and ``dup`` repeats one (vertex, hyperedge) incidence
in the raw list, which the 0/1 incidence matrix holds once."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from baselines_cases import WHOLE_MAX, assert_result, checksum, load, result, sample_idx, write_npz  # noqa: F401
from baselines_cases import raw_data as _hc_raw_data
from ce_cases import cotangent, perturb  # noqa: F401
from ce_cases import raw_data as _ce_raw_data

# name: layers, heads, row normalisation, self-loop hyperedges, training mode, sizes.  ``reseed`` moves a case to another seed where the
# first one puts a relu pre-activation of the float64 restatement within RELU_MARGIN of its kink (found on the CPU with the
# restatement alone: tests/test_unigcnii_reference.py::test_cases_keep_clear_of_the_relu_kink asserts it for every case)
CASES = {
    "uni_L1_h1":            dict(L=1, heads=1),
    "uni_L2_h1":            dict(L=2, heads=1),
    "uni_L4_h2":            dict(L=4, heads=2),
    "uni_L2_norm":          dict(L=2, heads=1, use_norm=True),
    "uni_L2_noself":        dict(L=2, heads=2, self_loops=False, dup=True),
    "uni_L2_noself_norm":   dict(L=2, heads=1, self_loops=False, dup=True, use_norm=True),
    "uni_L2_train":         dict(L=2, heads=1, train=True),
    "uni_L4_h2_norm_train": dict(L=4, heads=2, use_norm=True, train=True),
    # (the Cora-shaped case draws its hyperedges as tests/baselines_cases.py does -- one singleton hyperedge: the reference's
    #  Add_Self_Loops fails on a vertex that is alone in two)
    "cora_unigcnii":        dict(L=2, heads=2, n_v=2708, n_e=1579, F=1433, hidden=32, C=7, bow=True, empty=False, isolated=0),
}
FILES = {"baselines_unigcnii": [k for k in CASES if not k.startswith("cora")],
         "baselines_unigcnii_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT = 0.2                # fixed by the model, whatever --dropout says
RELU_MARGIN = 1e-6           # smallest |pre-activation| / (largest of its row): an order above the rounding of fp32 sums


def spec(name):
    c = dict(n_v=60, n_e=25, F=12, hidden=16, C=4, use_norm=False, self_loops=True, dup=False, train=False, bow=False,
             interior=(7, 30), trailing=4)
    c.update(CASES[name])
    c["seed"] = 4000 + sorted(CASES).index(name) + 100 * c.pop("reseed", 0)
    c["d"] = c["hidden"] * c["heads"]
    return c


def args_of(c):
    return SimpleNamespace(method="UniGCNII", All_num_layers=c["L"], dropout=0.5, MLP_hidden=c["hidden"], heads=c["heads"],
                           num_features=c["F"], num_classes=c["C"], UniGNN_use_norm=c["use_norm"], add_self_loop=c["self_loops"],
                           UniGNN_degV=0, UniGNN_degE=0, lr=0.001, wd=0.0)


def raw_data(c):
    """(x float64 [n_v, F], block edge list int64, n_v, n_e); ``dup``: the first V->E incidence once more, in both halves."""
    x, block, n_v, n_e = _hc_raw_data(c) if "isolated" in c else _ce_raw_data(c)
    if c["dup"]:
        v, e = block[0, 0], block[1, 0]
        assert v < n_v <= e
        block = np.concatenate([block, np.array([[v, e], [e, v]])], axis=1)
    return x, block, n_v, n_e


def masks(c):
    """Explicit dropout factors of a training-mode case: [n_v, F] for the input, then one [n_v, d] per conv and one for the last Linear."""
    if not c["train"]:
        return []
    rng = np.random.default_rng(c["seed"] + 11)
    shapes = [(c["n_v"], c["F"])] + [(c["n_v"], c["d"])] * (c["L"] + 1)
    return [(rng.random(s) >= DROPOUT) / (1.0 - DROPOUT) for s in shapes]
