"""CPU: the UniGNN baselines against what the REFERENCE computed (tests/golden/baselines_unignn*.npz, recorded by
tools/gen_unignn_fixtures.py from the cases of tests/unignn_cases.py): the product's initial parameters and state_dict layout (checksum
of the reference's draw under torch.manual_seed), and the float64 restatement tests/unignn_oracle.py on every case to 2e-5 -- output,
d/dx and every parameter gradient, in eval mode and in training mode with explicit dropout factors; every case's distance from the relu
and leaky-relu kinks.  Where the reference is importable (oracle/ref_shim.py) the fixtures are also regenerated and compared byte for
byte."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unigcnii_oracle as pre  # noqa: E402   (the float64 preprocessing: dense incidence, degrees, pairs)
import unignn_cases as gc  # noqa: E402
import unignn_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: f for f, names in gc.FILES.items() for name in names}


def _fx(name):
    return gc.load(FILE_OF[name])


def product_model(c, fx, name):
    """The product's module for the case, drawn under the case's seed, on the recorded pairs and scales (CPU: construction only)."""
    from allset_amd.baselines import UniGATConv, UniGNN
    args = gc.args_of(c)
    args.degV, args.degE = torch.from_numpy(fx[f"{name}/degV"]), torch.from_numpy(fx[f"{name}/degE"])
    pairs = torch.from_numpy(fx[f"{name}/pairs"]).long()
    torch.manual_seed(c["seed"])
    if c["kind"] == "conv":
        return UniGATConv(args, c["F"], c["hidden"], heads=c["heads"], dropout=0.0, skip_sum=True), args, pairs
    return UniGNN(args, nfeat=c["F"], nhid=c["hidden"], nclass=c["C"], nlayer=c["L"], nhead=c["heads"], V=pairs[0], E=pairs[1]), args, pairs


def oracle_inputs(c):
    """The restatement's own preprocessing of the case's raw data: ``(x, V, E, degV, degE)`` in float64."""
    x, block, n_v, n_e = gc.raw_data(c)
    v2e = torch.from_numpy(block[:, block[0] < n_v])
    if c["self_loops"]:                                      # one singleton hyperedge per vertex that is not already alone in one
        sizes = torch.bincount(v2e[1])
        alone = set(v2e[0][sizes[v2e[1]] == 1].tolist())
        new_v = torch.tensor([v for v in range(n_v) if v not in alone])
        v2e = torch.cat([v2e, torch.stack([new_v, int(v2e[1].max()) + 1 + torch.arange(new_v.numel())])], dim=1)
    H = pre.dense_incidence(v2e, n_v)
    V, E = pre.pairs(H)
    degV, degE = pre.degrees(H)
    return torch.from_numpy(x), V, E, degV, degE


def oracle_run(c, fx, name, sd64=None, masks=None):
    """The restatement on the case: ``(output, x leaf, parameter leaves, kink margins)``."""
    x, V, E, degV, degE = oracle_inputs(c)
    if sd64 is None:
        sd64 = gc.perturb(product_model(c, fx, name)[0].state_dict(), c)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = x.clone().requires_grad_(True)
    margins = []
    if c["kind"] == "conv":
        out = orc.conv("UniGAT", sd, xo, V, E, degV, degE, c, margins, skip_sum=True)
    else:
        if masks is None:
            masks = [torch.from_numpy(m) for m in gc.masks(c)] or None
        out = orc.forward(sd, xo, V, E, degV, degE, c, masks, margins)
    G = torch.from_numpy(gc.cotangent(c, out.shape[0]))
    (out * G).sum().backward()
    return out, xo, sd, margins


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    c = gc.spec(name)
    fx = _fx(name)
    model = product_model(c, fx, name)[0]
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert gc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
    if c["kind"] == "model":
        assert next(iter(model.state_dict())).startswith("conv_out.")


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_oracle_equals_recorded_reference(name):
    c = gc.spec(name)
    fx = _fx(name)
    out, xo, sd, _ = oracle_run(c, fx, name)
    gc.assert_result(out, fx, name, "out", rtol=2e-5, atol=2e-5)
    gc.assert_result(xo.grad, fx, name, "grad_x", rtol=2e-5, atol=2e-5)
    nograd = {str(s) for s in fx[f"{name}/nograd"]}
    assert nograd == {k for k in sd if k.endswith("att_v")}                       # unused in the reference: grad None
    for k, p in sd.items():
        if k in nograd:
            assert p.grad is None
        else:
            gc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=2e-5, atol=2e-5 * max(1.0, float(p.grad.abs().max())))


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_cases_keep_clear_of_the_kinks(name):
    """The a-priori criterion of every fp32 comparison with these cases (tests/test_gpu_unignn.py), from the restatement alone: no relu
    pre-activation and no attention logit within RELU_MARGIN of 0, relative to the largest of its row / of the logits."""
    c = gc.spec(name)
    _, _, _, margins = oracle_run(c, _fx(name), name)
    print("margins:", ["%.3e" % m for m in margins])
    n_relu = (c["L"] - 1) if (c["kind"] == "model" and c["activation"] == "relu") else 0
    n_att = (c["L"] if c["kind"] == "model" else 1) if c["model"] == "UniGAT" else 0
    assert len(margins) == n_relu + n_att and min(margins, default=1.0) > gc.RELU_MARGIN


def test_cases_cover_what_the_issue_lists():
    S = {n: gc.spec(n) for n in gc.CASES}
    models = {c["model"] for c in S.values() if c["kind"] == "model" and c["L"] == 2}
    assert models == {"UniGCN", "UniGCN2", "UniGIN", "UniSAGE", "UniGAT"}
    assert {c["heads"] for c in S.values()} >= {1, 2} and {c["first"] for c in S.values()} == {"mean", "sum"}
    assert any(c["model"] == "UniSAGE" and c["second"] == "mean" for c in S.values())
    assert {c["use_norm"] for c in S.values()} == {True, False}
    assert any(c["kind"] == "conv" for c in S.values()) and any(c["L"] == 3 for c in S.values())
    assert any(c["train"] for c in S.values()) and any(c["activation"] == "prelu" for c in S.values())
    assert any(not c["self_loops"] and c["dup"] and c["model"] == "UniGAT" for c in S.values())
    assert any(not c["self_loops"] and c["use_norm"] for c in S.values())
    assert any(c["C"] % 4 for c in S.values())                                    # the unfused last conv


def test_recorded_cases_have_the_quirks():
    name = "gin_L2_noself_norm"
    fx, c = _fx(name), gc.spec(name)
    pairs = fx[f"{name}/pairs"]
    deg = np.bincount(pairs[0], minlength=c["n_v"])
    iso = set(np.flatnonzero(deg == 0).tolist())
    assert set(c["interior"]) <= iso and {c["n_v"] - 1, c["n_v"] - c["trailing"]} <= iso
    assert len({(int(v), int(e)) for v, e in pairs.T}) == pairs.shape[1]           # the repeated incidence is there once
    x, V, E, degV, degE = oracle_inputs(c)
    np.testing.assert_array_equal(torch.stack([V, E]).numpy(), pairs.astype(np.int64))
    np.testing.assert_allclose(degV.numpy(), fx[f"{name}/degV"], rtol=1e-6)


def test_refusals():
    from allset_amd.baselines import UniGATConv, UniGCNConv, UniGNN, UniSAGEConv
    c = gc.spec("gcn_L2_h1")
    args = gc.args_of(c)
    args.first_aggregate = "max"
    with pytest.raises(NotImplementedError, match="first_aggregate"):
        UniGCNConv(args, 4, 4, heads=1)
    args = gc.args_of(c)
    args.second_aggregate = "max"
    with pytest.raises(NotImplementedError, match="second_aggregate"):
        UniSAGEConv(args, 4, 4, heads=1)
    args = gc.args_of(c)
    with pytest.raises(NotImplementedError, match="attention coefficients"):
        UniGATConv(args, 4, 4, heads=1, dropout=0.1)
    args.attn_drop, args.model_name = 0.2, "UniGAT"
    with pytest.raises(NotImplementedError, match="attention coefficients"):
        UniGNN(args, 4, 4, 3, 2, 1, None, None)


@pytest.mark.skipif(not __import__("oracle.ref_shim", fromlist=["x"]).available(), reason="needs the reference sources")
def test_fixtures_regenerate_byte_for_byte():
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_unignn_fixtures.py"), "--check"], capture_output=True,
                         text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
