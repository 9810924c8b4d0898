"""CPU: the CEGCN baseline against what the REFERENCE computed (tests/golden/baselines_ce*.npz, recorded by tools/gen_ce_fixtures.py
from the cases of tests/ce_cases.py): the product's initial parameters and state_dict layout (checksum of the reference's draw under
torch.manual_seed), and the float64 restatement tests/ce_oracle.py on every case to 2e-5 -- clique expansion, gcn_norm, logits,
d/dx and every parameter gradient, in eval mode and in training mode with explicit dropout factors.  Where the reference is
importable (oracle/ref_shim.py) the fixtures are also regenerated and compared byte for byte."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_cases as cc  # noqa: E402
import ce_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: f for f, names in cc.FILES.items() for name in names}


def _fx(name):
    return cc.load(FILE_OF[name])


def _canon(ei, w):
    ei, w = np.asarray(ei), np.asarray(w)
    order = np.lexsort((ei[1], ei[0]))
    return ei[:, order], w[order]


def _product_model(c):
    from allset_amd.train import build_model
    from types import SimpleNamespace
    torch.manual_seed(c["seed"])
    return build_model(cc.args_of(c), SimpleNamespace(clique_expansion=True))


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    c = cc.spec(name)
    fx = _fx(name)
    model = _product_model(c)
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert cc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_oracle_preprocessing_equals_reference(name):
    """Pairs in one direction, multiplicities, no pair from a size-1 hyperedge, N = max id + 1 (trailing ids get no loop)."""
    c = cc.spec(name)
    fx = _fx(name)
    x, block, n_v, _ = cc.raw_data(c)
    v2e = torch.from_numpy(block[:, block[0] < n_v])
    pairs, mult = orc.clique_expansion(v2e)
    ref_pairs, ref_m = _canon(fx[f"{name}/pairs"], fx[f"{name}/pair_norm"])
    np.testing.assert_array_equal(pairs.numpy(), ref_pairs)
    np.testing.assert_array_equal(mult.numpy().astype(np.float32), ref_m)
    assert ref_m.max() >= 3.0 and bool((ref_pairs[0] < ref_pairs[1]).all())
    ei, w = orc.gcn_norm(pairs, mult)
    got_ei, got_w = _canon(ei.numpy(), w.numpy())
    ref_ei, ref_w = _canon(fx[f"{name}/edge_index"], fx[f"{name}/norm"])
    np.testing.assert_array_equal(got_ei, ref_ei)
    np.testing.assert_allclose(got_w, ref_w, rtol=1e-6, atol=0)
    assert int(ref_ei.max()) + 1 == n_v - c["trailing"] or c["trailing"] == 0


def _oracle(c, fx, name):
    ei = torch.from_numpy(fx[f"{name}/edge_index"])
    w = torch.from_numpy(fx[f"{name}/norm"]).double()
    x, _, _, _ = cc.raw_data(c)
    sd = {k: (v.requires_grad_(True) if v.is_floating_point() else v) for k, v in cc.perturb(_product_model(c).state_dict(), c).items()}
    xo = torch.from_numpy(x).requires_grad_(True)
    masks = [torch.from_numpy(m) for m in cc.masks(c)] or None
    lo = orc.cegcn_forward(sd, xo, ei, w, max(c["L"], 2), masks, bn=c["norm"] == "bn", training=c["train"])
    G = torch.from_numpy(cc.cotangent(c, lo.shape[0]))
    (lo * G).sum().backward()
    return lo, xo, sd


@pytest.mark.parametrize("name", sorted(cc.CASES))
def test_oracle_equals_recorded_reference(name):
    c = cc.spec(name)
    fx = _fx(name)
    lo, xo, sd = _oracle(c, fx, name)
    cc.assert_result(lo, fx, name, "logits", rtol=2e-5, atol=2e-5)
    cc.assert_result(xo.grad, fx, name, "grad_x", rtol=2e-5, atol=2e-5)
    for k, p in sd.items():
        if p.requires_grad and not k.endswith(("running_mean", "running_var")):
            cc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=2e-5, atol=2e-5 * max(1.0, float(p.grad.abs().max())))


@pytest.mark.skipif(not __import__("oracle.ref_shim", fromlist=["x"]).available(), reason="needs the reference sources")
def test_fixtures_regenerate_byte_for_byte():
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_ce_fixtures.py"), "--check"], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
