"""CPU: the UniGCNII baseline against what the REFERENCE computed (tests/golden/baselines_unigcnii*.npz, recorded by
tools/gen_unigcnii_fixtures.py from the cases of tests/unigcnii_cases.py): the product's initial parameters, state_dict layout and
parameter groups (checksum of the reference's draw under torch.manual_seed), and the float64 restatement tests/unigcnii_oracle.py on
every case to 2e-5 -- logits, d/dx and every parameter gradient, in eval mode and in training mode with explicit dropout factors; the
restatement's sparse form against its dense-H form; every case's distance from the relu kink.  Where the reference is importable
(oracle/ref_shim.py) the fixtures are also regenerated and compared byte for byte."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unigcnii_cases as uc  # noqa: E402
import unigcnii_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: f for f, names in uc.FILES.items() for name in names}


def _fx(name):
    return uc.load(FILE_OF[name])


def _product_model(c, fx, name):
    from allset_amd.train import build_model
    torch.manual_seed(c["seed"])
    args = uc.args_of(c)
    args.UniGNN_degV, args.UniGNN_degE = torch.from_numpy(fx[f"{name}/degV"]), torch.from_numpy(fx[f"{name}/degE"])
    pairs = torch.from_numpy(fx[f"{name}/pairs"]).long()
    data = SimpleNamespace(edge_index=pairs, UniGNN_sizes=(c["n_v"], args.UniGNN_degE.shape[0]))
    return build_model(args, data)


@pytest.mark.parametrize("name", sorted(uc.CASES))
def test_initial_parameters_layout_and_groups_equal_reference(name):
    c = uc.spec(name)
    fx = _fx(name)
    model = _product_model(c, fx, name)
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert uc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
    names = {id(p): k for k, p in model.named_parameters()}
    assert [names[id(p)] for p in model.reg_params] == [str(s) for s in fx[f"{name}/reg_params"]]
    assert [names[id(p)] for p in model.non_reg_params] == [str(s) for s in fx[f"{name}/non_reg_params"]]


def oracle_run(c, fx, name, sd64=None, masks=None, dense=False):
    """The restatement on the case's inputs, its own preprocessing included: ``(logits, x leaf, parameter leaves, relu margins)``."""
    x, block, n_v, n_e = uc.raw_data(c)
    v2e = torch.from_numpy(block[:, block[0] < n_v])
    if c["self_loops"]:                                      # one singleton hyperedge per vertex that is not already alone in one
        sizes = torch.bincount(v2e[1])
        alone = set(v2e[0][sizes[v2e[1]] == 1].tolist())
        new_v = torch.tensor([v for v in range(n_v) if v not in alone])
        v2e = torch.cat([v2e, torch.stack([new_v, int(v2e[1].max()) + 1 + torch.arange(new_v.numel())])], dim=1)
    H = orc.dense_incidence(v2e, n_v)
    V, E = orc.pairs(H)
    degV, degE = orc.degrees(H)
    if sd64 is None:
        sd64 = uc.perturb(_product_model(c, fx, name).state_dict(), c)
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = torch.from_numpy(x).requires_grad_(True)
    if masks is None:
        masks = [torch.from_numpy(m) for m in uc.masks(c)] or None
    margins = []
    lo = orc.forward(sd, xo, V, E, degV, degE, c["L"], c["use_norm"], masks, margins, H=H if dense else None)
    G = torch.from_numpy(uc.cotangent(c, lo.shape[0]))
    (lo * G).sum().backward()
    return lo, xo, sd, margins


@pytest.mark.parametrize("name", sorted(uc.CASES))
def test_oracle_equals_recorded_reference(name):
    c = uc.spec(name)
    fx = _fx(name)
    lo, xo, sd, _ = oracle_run(c, fx, name)
    uc.assert_result(lo, fx, name, "logits", rtol=2e-5, atol=2e-5)
    uc.assert_result(xo.grad, fx, name, "grad_x", rtol=2e-5, atol=2e-5)
    for k, p in sd.items():
        uc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=2e-5, atol=2e-5 * max(1.0, float(p.grad.abs().max())))
    assert len(sd) == c["L"] + 4


@pytest.mark.parametrize("name", sorted(uc.CASES))
def test_cases_keep_clear_of_the_relu_kink(name):
    """The a-priori criterion of every fp32 comparison with these cases (tests/test_gpu_unigcnii.py), from the restatement alone."""
    c = uc.spec(name)
    _, _, _, margins = oracle_run(c, _fx(name), name)
    print("relu margins:", ["%.3e" % m for m in margins])
    assert len(margins) == c["L"] + 1 and min(margins) > uc.RELU_MARGIN


@pytest.mark.parametrize("name", [n for n in sorted(uc.CASES) if not n.startswith("cora")])
def test_sparse_form_equals_dense_form(name):
    c = uc.spec(name)
    fx = _fx(name)
    a, xa, sda, _ = oracle_run(c, fx, name)
    b, xb, sdb, _ = oracle_run(c, fx, name, dense=True)
    torch.testing.assert_close(a, b, rtol=1e-11, atol=1e-11)
    torch.testing.assert_close(xa.grad, xb.grad, rtol=1e-10, atol=1e-10)
    for k in sda:
        torch.testing.assert_close(sda[k].grad, sdb[k].grad, rtol=1e-10, atol=1e-10)


def test_recorded_cases_have_the_quirks():
    fx = _fx("uni_L2_noself_norm")
    degV, pairs = fx["uni_L2_noself_norm/degV"].reshape(-1), fx["uni_L2_noself_norm/pairs"]
    c = uc.spec("uni_L2_noself_norm")
    deg = np.bincount(pairs[0], minlength=c["n_v"])
    iso = np.flatnonzero(deg == 0)
    assert set(c["interior"]) <= set(iso.tolist()) and {c["n_v"] - 1, c["n_v"] - c["trailing"]} <= set(iso.tolist())
    assert (degV[iso] == 1.0).all()
    assert len({(int(v), int(e)) for v, e in pairs.T}) == pairs.shape[1]           # the repeated incidence is there once
    assert (np.diff(pairs[0].astype(np.int64) * (pairs[1].max() + 1) + pairs[1]) > 0).all()       # sorted by (v, e)


@pytest.mark.skipif(not __import__("oracle.ref_shim", fromlist=["x"]).available(), reason="needs the reference sources")
def test_fixtures_regenerate_byte_for_byte():
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_unigcnii_fixtures.py"), "--check"], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
