"""The float64 restatement of the hypergraph attention conv (tests/hcha_attn_oracle.py) against what the reference's own
``HypergraphConv(use_attention=True)`` computed (tests/golden/baselines_hcha_attn.npz): output, d/dx and every parameter gradient to
1e-9 -- only the float64 summation order differs.  No GPU."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcha_attn_cases as hc  # noqa: E402
import hcha_attn_oracle as orc  # noqa: E402

TOL = dict(rtol=1e-9, atol=1e-9)


def initial_state(c):
    from allset_amd.baselines import HypergraphAttentionConv
    torch.manual_seed(c["seed"])
    return HypergraphAttentionConv(hc.F_IN, c["out"], heads=c["heads"], concat=c["concat"]).state_dict()


def oracle_case(c, softmax_by="vertex"):
    x, ei, w = hc.inputs(c)
    sd = {k: v.requires_grad_(True) for k, v in hc.perturb(initial_state(c), c).items()}
    xo = x.clone().requires_grad_(True)
    out = orc.conv(xo, sd["weight"], sd["att"], sd["bias"], ei, hc.N_E, c["heads"], concat=c["concat"], hyperedge_weight=w,
                   coef_mask=hc.coef_mask(c, ei.shape[1]), softmax_by=softmax_by)
    (out * hc.cotangent(c, out.shape[0])).sum().backward()
    return out.detach(), xo.grad, {k: v.grad for k, v in sd.items()}


@pytest.fixture(scope="module")
def fx():
    return hc.load(hc.FILE)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_equals_recorded_reference(fx, name):
    c = hc.spec(name)
    out, gx, grads = oracle_case(c)
    torch.testing.assert_close(out, torch.from_numpy(fx[f"{name}/out"]), **TOL)
    torch.testing.assert_close(gx, torch.from_numpy(fx[f"{name}/grad_x"]), **TOL)
    assert sorted(grads) == sorted(k.split("grad:")[1] for k in fx if k.startswith(f"{name}/grad:"))
    for k, g in grads.items():
        torch.testing.assert_close(g, torch.from_numpy(fx[f"{name}/grad:{k}"]), msg=lambda m, k=k: f"{k}: {m}", **TOL)
    if c["isolated"]:
        assert torch.equal(out[-c["isolated"]:], (hc.perturb(initial_state(c), c)["bias"]).expand(c["isolated"], -1))


def test_restatement_sees_the_normalisation_axis(fx):
    """The same comparison with the softmax grouped by hyperedge instead of by vertex must fail."""
    c = hc.spec("h4_concat")
    out, _, _ = oracle_case(c, softmax_by="edge")
    with pytest.raises(AssertionError):
        torch.testing.assert_close(out, torch.from_numpy(fx["h4_concat/out"]), **TOL)
