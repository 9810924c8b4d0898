"""CPU: the HAN baseline against what the REFERENCE computed (tests/golden/baselines_han*.npz, recorded by tools/gen_han_fixtures.py from
the cases of tests/han_cases.py).  The fixtures come from the reference's own DGL_HAN/model.py classes with a stand-in for
``dgl.nn.pytorch.GATConv`` (``dgl`` is not installable here): they pin the composition, the parameter creation order and the
``state_dict`` layout; the ``GATConv`` itself is pinned only by the restatement of DGL 0.7.1's documented formulas in
tests/han_oracle.py.  Checked here: the product's initial parameters and layout (checksum of the reference's draw under
``torch.manual_seed``), the functional float64 restatement on every case to 2e-5 -- logits, d/dx and every parameter gradient, in eval
mode and in training mode with explicit dropout factors -- and every case's distance from the leaky-relu kink.  Where the reference is
importable the fixtures are also regenerated and compared byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_cases as hc  # noqa: E402
import han_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: f for f, names in hc.FILES.items() for name in names}
TOL = dict(rtol=2e-5, atol=2e-5)


def product_model(c):
    from allset_amd.han import HAN
    torch.manual_seed(c["seed"])
    return HAN(num_meta_paths=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=hc.DROPOUT)


def oracle_run(c, sd64=None, masks="case"):
    """The restatement on the case: ``(logits, x leaf, parameter leaves, kink margin)``."""
    x, pairs, n_v, n_e = hc.raw_data(c)
    graphs = [(torch.from_numpy(r), torch.from_numpy(cc)) for r, cc in hc.dense_metapath_edges(pairs, n_v, n_e)]
    if sd64 is None:
        sd64 = hc.perturb(product_model(c).state_dict(), c)
    if isinstance(masks, str):
        masks = hc.masks(c, [g[0].numel() for g in graphs])
        if masks is not None:
            masks = [[tuple(torch.from_numpy(m) for m in pair) for pair in layer] for layer in masks]
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = torch.from_numpy(x).clone().requires_grad_(True)
    report = []
    out = orc.han_forward(sd, graphs, n_v + n_e, xo, len(c["heads"]), masks, report)
    (out * torch.from_numpy(hc.cotangent(c, n_v + n_e))).sum().backward()
    return out, xo, sd, min(report)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    c = hc.spec(name)
    fx = hc.load(FILE_OF[name])
    model = product_model(c)
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert hc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
    keys = list(model.state_dict())
    assert keys[:4] == ["layers.0.gat_layers.0.attn_l", "layers.0.gat_layers.0.attn_r", "layers.0.gat_layers.0.bias",
                        "layers.0.gat_layers.0.fc.weight"]
    assert "layers.0.semantic_attention.project.0.weight" in keys and "layers.0.semantic_attention.project.2.weight" in keys
    assert float(model.layers[0].gat_layers[0].bias.detach().abs().max()) == 0.0


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_equals_reference(name):
    c = hc.spec(name)
    fx = hc.load(FILE_OF[name])
    out, xo, sd, margin = oracle_run(c)
    print(f"{name}: kink margin {margin:.3e} (recorded {float(fx[name + '/margin']):.3e})")
    assert margin > hc.KINK_MARGIN and float(fx[f"{name}/margin"]) > hc.KINK_MARGIN
    hc.assert_result(out, fx, name, "out", **TOL)
    hc.assert_result(xo.grad, fx, name, "grad_x", **TOL)
    for k, v in sd.items():
        hc.assert_result(v.grad, fx, name, f"grad:{k}", **TOL)


def test_cases_cover_what_the_issue_lists():
    specs = [hc.spec(n) for n in hc.CASES]
    assert {h for c in specs for h in c["heads"]} >= {1, 2, 8}
    assert {len(c["heads"]) for c in specs} >= {1, 2}
    assert any(c["train"] for c in specs) and any(not c["train"] for c in specs)
    assert any(c["n_v"] == 2708 and c["n_e"] == 1579 and c["F"] == 1433 for c in specs)
    c = hc.spec("han_h2_L1")
    x, pairs, n_v, n_e = hc.raw_data(c)
    sizes = np.bincount(np.unique(pairs[0] * n_e + pairs[1]) % n_e, minlength=n_e)
    assert (sizes == 1).sum() >= 2                                                        # size-1 hyperedges
    assert not np.isin(np.arange(n_v - c["isolated"], n_v), pairs[0]).any()               # vertices in no hyperedge
    assert pairs.shape[1] > np.unique(pairs[0] * n_e + pairs[1]).size                     # duplicate incidences
    (r, cc), _ = hc.dense_metapath_edges(pairs, n_v, n_e)
    assert np.bincount(r[r == cc], minlength=n_v + n_e).max() == 2                        # doubled self-loops


def test_explicit_dropout_factors_matter():
    """The training-mode fixtures would not notice a conv that ignored its factors unless they changed the result."""
    c = hc.spec("han_h2_L1_train")
    a = oracle_run(c)[0]
    b = oracle_run(c, masks=None)[0]
    assert float((a - b).abs().max()) > 1e-2


def test_fixtures_regenerate_byte_for_byte():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_han_fixtures as gen
    if not gen.available():
        pytest.skip("the reference's sources are not on this machine")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_han_fixtures.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
