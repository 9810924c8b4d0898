"""CPU: the HGNN / HCHA / HNHN baselines against what the REFERENCE computed (tests/golden/baselines_*.npz, recorded by
tools/gen_baseline_fixtures.py from the cases of tests/baselines_cases.py): the driver's preprocessing and HNHN norms, the initial
parameters and state_dict layout, and the float64 restatement tests/baselines_oracle.py on every case to 2e-5 -- eval mode, training
mode with explicit dropout factors, and the NaN gradients of HNHN at isolated vertices.  Where the reference is importable
(oracle/ref_shim.py) the fixtures are also regenerated and compared byte for byte."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baselines_cases as bc  # noqa: E402
import baselines_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: f for f, names in bc.FILES.items() for name in names}


def _fx(name):
    return bc.load(FILE_OF[name])


def _canon(ei):
    ei = np.asarray(ei)
    return ei[:, np.lexsort((ei[1], ei[0]))]


def _product_model(c):
    from allset_amd.baselines import HCHA, HNHN
    torch.manual_seed(c["seed"])
    return (HNHN if c["method"] == "HNHN" else HCHA)(bc.args_of(c))


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_preprocessing_and_norms_equal_reference(name):
    from allset_amd.train import HypergraphData, preprocess
    c = bc.spec(name)
    fx = _fx(name)
    x, block, n_v, n_e = bc.raw_data(c)
    args = bc.args_of(c)
    data = HypergraphData(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e])
    data = preprocess(args, data)
    ref_ei = fx[f"{name}/edge_index"]
    np.testing.assert_array_equal(_canon(data.edge_index.numpy()), _canon(ref_ei))       # (order within a vertex: unstable sort there)
    if c["method"] == "HNHN":
        for k in ("D_e_alpha", "D_v_alpha_inv", "D_v_beta", "D_e_beta_inv"):
            np.testing.assert_allclose(getattr(data, k).numpy(), fx[f"{name}/norm:{k}"], rtol=1e-6, err_msg=k)
    else:
        D, B = orc.hcha_scales(torch.from_numpy(ref_ei), n_v, c["sym"])
        torch.testing.assert_close(data.HCHA_D.double(), D, rtol=1e-6, atol=0)
        torch.testing.assert_close(data.HCHA_B.double(), B, rtol=1e-6, atol=0)


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    c = bc.spec(name)
    fx = _fx(name)
    model = _product_model(c)
    spec = [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()]
    assert spec == [str(s) for s in fx[f"{name}/spec"]]
    assert bc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])


def _oracle(c, fx, name):
    ei = torch.from_numpy(fx[f"{name}/edge_index"])
    x, _, n_v, _ = bc.raw_data(c)
    sd = {k: v.requires_grad_(True) for k, v in bc.perturb(_product_model(c).state_dict(), c).items()}
    xo = torch.from_numpy(x).requires_grad_(True)
    masks = [torch.from_numpy(m) for m in bc.masks(c)] or None
    if c["method"] == "HNHN":
        norms = {k: torch.from_numpy(v) for k, v in orc.hnhn_norms_dense(ei, n_v, -1.5, -0.5).items()}
        for k, v in norms.items():                               # the oracle's norms are the reference's
            np.testing.assert_allclose(v.numpy().astype(np.float32), fx[f"{name}/norm:{k}"], rtol=1e-6, err_msg=k)
        lo = orc.hnhn_forward(sd, xo, ei, norms, c["L"], c["nonlinear"], masks)
    else:
        lo = orc.hcha_forward(sd, xo, ei, max(c["L"], 2), c["sym"], masks)
    G = torch.from_numpy(bc.cotangent(c, lo.shape[0]))
    (lo * G).sum().backward()
    return lo, xo, sd


@pytest.mark.parametrize("name", sorted(bc.CASES))
def test_oracle_equals_recorded_reference(name):
    c = bc.spec(name)
    fx = _fx(name)
    lo, xo, sd = _oracle(c, fx, name)
    nan = c["method"] == "HNHN" and c["isolated"] > 0
    bc.assert_result(lo, fx, name, "logits", rtol=2e-5, atol=2e-5)
    bc.assert_result(xo.grad, fx, name, "grad_x", rtol=2e-5, atol=2e-5, equal_nan=nan)
    for k, p in sd.items():
        bc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=2e-5, atol=2e-5 * max(1.0, float(p.grad.abs().nan_to_num().max())),
                         equal_nan=nan)
    if nan:                                                      # the reference's NaN gradients
        kind, v = bc.result(fx, name, "grad:convs.0.weight_v2e.weight")
        assert np.isnan(v if kind == "whole" else v[1]).all()
        assert np.isnan(bc.result(fx, name, "grad_x")[1][-c["isolated"]:]).all()


@pytest.mark.skipif(not __import__("oracle.ref_shim", fromlist=["x"]).available(), reason="needs the reference sources")
def test_fixtures_regenerate_byte_for_byte(tmp_path):
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_baseline_fixtures.py"), "--check"], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.skipif(not __import__("oracle.ref_shim", fromlist=["x"]).available(), reason="needs the reference sources")
@pytest.mark.parametrize("method", ["HCHA", "HNHN"])
def test_state_dict_equals_live_reference(method):
    from oracle import ref_shim
    _, ref_models = ref_shim.import_reference()
    for L in (1, 2, 3):
        c = bc.spec("hnhn_L2" if method == "HNHN" else "hcha_L2")
        c["L"] = L
        args = bc.args_of(c)
        torch.manual_seed(c["seed"])
        ref = getattr(ref_models, method)(args).state_dict()
        ours = _product_model(c).state_dict()                   # (seeds with c["seed"] too)
        assert [(k, v.shape, v.dtype) for k, v in ours.items()] == [(k, v.shape, v.dtype) for k, v in ref.items()]
        assert all(torch.equal(ours[k], ref[k]) for k in ref)
