"""The cases of the CEGAT reference fixtures (tests/golden/baselines_cegat*.npz, written by tools/gen_cegat_fixtures.py): every input
is rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.  Raw data, file format, checksum, sampling
of large results and the comparison helper are those of tests/ce_cases.py / tests/baselines_cases.py: hyperedges of 2..8 members,
a few of one (they add no pair), a pair shared by three more hyperedges, ``interior`` and the last ``trailing`` vertex ids in no
hyperedge (both kinds get a GAT self-loop: their output is their own transformed row)."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from baselines_cases import WHOLE_MAX, assert_result, checksum, load, result, sample_idx, write_npz  # noqa: F401
from ce_cases import cotangent, perturb, raw_data  # noqa: F401

# name: layers, heads, output heads, normalisation, training mode, sizes.  ``reseed``: moves the case to another seed where the first
# one puts a pre-activation of some conv within 1e-5 of leaky_relu's kink (the GPU comparison in fp32 asserts that margin from the
# float64 restatement; tests/test_gpu_cegat.py)
CASES = {
    "cegat_L1_h1_o1":    dict(L=1, heads=1, oheads=1),
    "cegat_L1_h4_o2":    dict(L=1, heads=4, oheads=2),
    "cegat_L2_h1_o2":    dict(L=2, heads=1, oheads=2),
    "cegat_L2_h4_o1":    dict(L=2, heads=4, oheads=1),
    "cegat_L3_h1":       dict(L=3, heads=1, oheads=1),
    "cegat_L2_bn":       dict(L=2, heads=1, oheads=2, norm="bn"),
    "cegat_L2_h4_train": dict(L=2, heads=4, oheads=2, train=True),
    "cegat_L3_bn_train": dict(L=3, heads=1, oheads=1, norm="bn", train=True),
    "cora_cegat":        dict(L=2, heads=4, oheads=1, reseed=5, n_v=2708, n_e=1579, F=1433, hidden=16, C=7, bow=True, interior=(), trailing=3),
}
FILES = {"baselines_cegat": [k for k in CASES if not k.startswith("cora")],
         "baselines_cegat_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT = 0.5


def spec(name):
    c = dict(n_v=60, n_e=25, F=12, hidden=16, C=4, norm="ln", train=False, bow=False, interior=(7, 30), trailing=4)
    c.update(CASES[name])
    c["seed"] = 3000 + sorted(CASES).index(name) + 100 * c.pop("reseed", 0)
    return c


def args_of(c):
    return SimpleNamespace(method="CEGAT", All_num_layers=c["L"], dropout=DROPOUT, MLP_hidden=c["hidden"], num_features=c["F"],
                           num_classes=c["C"], normalization=c["norm"], heads=c["heads"], output_heads=c["oheads"])


def n_convs(c):
    return max(c["L"], 2)


def masks(c):
    """Explicit dropout factors, one [n_v, width of conv i's output] array per dropout site of a training-mode case."""
    if not c["train"]:
        return []
    rng = np.random.default_rng(c["seed"] + 11)
    widths = [c["heads"] * c["hidden"]] + [c["hidden"]] * (n_convs(c) - 2)
    return [(rng.random((c["n_v"], w)) >= DROPOUT) / (1.0 - DROPOUT) for w in widths]


def perturbed(sd, c):
    """``ce_cases.perturb`` of a CEGAT ``state_dict`` (float64), with every ``lin_r.weight`` equal to its conv's ``lin_l.weight``: the
    two names are one tensor."""
    out = perturb(sd, c)
    return {k: (out[k.replace("lin_r", "lin_l")] if "lin_r" in k else v) for k, v in out.items()}
