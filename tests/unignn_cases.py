"""The cases of the UniGNN reference fixtures (tests/golden/baselines_unignn*.npz, written by tools/gen_unignn_fixtures.py): every input is
rebuilt here from fixed seeds, so the fixtures hold only what the reference computed.  Raw data, file format, checksum, sampling of
large results and the comparison helper are those of tests/unigcnii_cases.py: hyperedges of 2..8 members, a few of one, a member set
shared by three hyperedges, ``interior`` and the last ``trailing`` vertex ids in no hyperedge.  With ``self_loops`` (the driver's
default) every vertex gets a singleton hyperedge; without, the isolated vertices keep a zero row of the incidence matrix (a zero row
norm under ``use_norm``, an empty softmax in UniGAT) and ``dup`` repeats one (vertex, hyperedge) incidence in the raw list.

``kind`` 'model': the reference's ``UniGNN`` with the conv ``model``; 'conv': one ``UniGATConv(skip_sum=True)`` on its own."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from unigcnii_cases import WHOLE_MAX, assert_result, checksum, cotangent, load, perturb, raw_data, result, sample_idx, write_npz  # noqa: F401

# ``reseed`` moves a case to another seed where the first one puts a relu pre-activation or an attention logit of the float64
# restatement within RELU_MARGIN of its kink (tests/test_unignn_reference.py::test_cases_keep_clear_of_the_kinks asserts it), or
# draws a vertex that is alone in two hyperedges (the reference's Add_Self_Loops fails on it)
CASES = {
    "gcn_L2_h1":              dict(model="UniGCN", L=2, heads=1),
    "gcn_L2_h2_sum_norm":     dict(model="UniGCN", L=2, heads=2, first="sum", use_norm=True),
    "gcn_L2_prelu_c5":        dict(model="UniGCN", L=2, heads=1, activation="prelu", C=5),
    "gcn2_L2_h2_norm":        dict(model="UniGCN2", L=2, heads=2, use_norm=True),
    "gcn2_L3_h1_sum":         dict(model="UniGCN2", L=3, heads=1, first="sum"),
    "gin_L2_h2":              dict(model="UniGIN", L=2, heads=2, reseed=2),
    "gin_L2_noself_norm":     dict(model="UniGIN", L=2, heads=1, self_loops=False, dup=True, use_norm=True),
    "sage_L2_h1_mean2":       dict(model="UniSAGE", L=2, heads=1, second="mean"),
    "sage_L3_h2_norm_train":  dict(model="UniSAGE", L=3, heads=2, use_norm=True, train=True),
    "gat_L2_h1":              dict(model="UniGAT", L=2, heads=1),
    "gat_L2_h2_norm_c5":      dict(model="UniGAT", L=2, heads=2, use_norm=True, C=5, reseed=1),
    "gat_L2_noself_sum":      dict(model="UniGAT", L=2, heads=2, first="sum", self_loops=False, dup=True),
    "gat_L3_h2_prelu_train":  dict(model="UniGAT", L=3, heads=2, activation="prelu", train=True),
    "gin_L2_train":           dict(model="UniGIN", L=2, heads=1, train=True),
    "gatconv_skip":           dict(kind="conv", model="UniGAT", heads=2),
    "gatconv_skip_norm":      dict(kind="conv", model="UniGAT", heads=2, use_norm=True, self_loops=False, dup=True),
    "cora_unigat":            dict(model="UniGAT", L=2, heads=2, n_v=2708, n_e=1579, F=1433, hidden=32, C=7, bow=True, empty=False,
                                   isolated=0),
    "cora_unigin_norm":       dict(model="UniGIN", L=2, heads=2, use_norm=True, n_v=2708, n_e=1579, F=1433, hidden=32, C=7, bow=True,
                                   empty=False, isolated=0),
}
FILES = {"baselines_unignn": [k for k in CASES if not k.startswith("cora")],
         "baselines_unignn_cora": [k for k in CASES if k.startswith("cora")]}
DROPOUT, INPUT_DROP = 0.5, 0.6
RELU_MARGIN = 1e-6           # smallest |pre-activation| / (largest of its row; of the whole matrix for the attention logits)


def spec(name):
    c = dict(kind="model", n_v=60, n_e=25, F=12, hidden=16, C=4, L=2, use_norm=False, self_loops=True, dup=False, train=False, bow=False,
             interior=(7, 30), trailing=4, first="mean", second="sum", activation="relu")
    c.update(CASES[name])
    c["seed"] = 5000 + sorted(CASES).index(name) + 100 * c.pop("reseed", 0)
    c["d"] = c["hidden"] * c["heads"]
    if c["kind"] == "conv":                                  # one conv: F -> heads * hidden, skip_sum needs nothing else
        c["C"] = c["d"]
    return c


def args_of(c):
    """What the reference's convs read from ``args`` (``degV`` / ``degE`` are filled in by the caller)."""
    return SimpleNamespace(model_name=c["model"], first_aggregate=c["first"], second_aggregate=c["second"], use_norm=c["use_norm"],
                           attn_drop=0.0, activation=c["activation"], input_drop=INPUT_DROP, dropout=DROPOUT, degV=None, degE=None)


def masks(c):
    """Explicit dropout factors of a training-mode case: [n_v, F] for the input, then one [n_v, d] per hidden conv."""
    if not c["train"]:
        return []
    rng = np.random.default_rng(c["seed"] + 11)
    out = [(rng.random((c["n_v"], c["F"])) >= INPUT_DROP) / (1.0 - INPUT_DROP)]
    return out + [(rng.random((c["n_v"], c["d"])) >= DROPOUT) / (1.0 - DROPOUT) for _ in range(c["L"] - 1)]
