"""CPU: the CEGAT baseline against what the REFERENCE computed (tests/golden/baselines_cegat*.npz, recorded by
tools/gen_cegat_fixtures.py from the cases of tests/cegat_cases.py): the product's initial parameters and state_dict layout
(checksum of the reference's draw under torch.manual_seed), and the float64 restatement tests/cegat_oracle.py on every case to
2e-5 -- logits, d/dx and every parameter gradient, in eval mode and in training mode with explicit dropout factors.  Where the
reference is importable (oracle/ref_shim.py) the fixtures are also regenerated and compared byte for byte."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cegat_cases as gc  # noqa: E402
import cegat_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: f for f, names in gc.FILES.items() for name in names}


def _fx(name):
    return gc.load(FILE_OF[name])


def _product_model(c, fx, name):
    from allset_amd.train import build_model
    torch.manual_seed(c["seed"])
    data = SimpleNamespace(clique_expansion=True, edge_index=torch.from_numpy(fx[f"{name}/edge_index"]).long())
    return build_model(gc.args_of(c), data)


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    c = gc.spec(name)
    fx = _fx(name)
    model = _product_model(c, fx, name)
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert gc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])


def oracle_run(c, fx, name, sd64=None, masks=None):
    """The restatement on the case's inputs: ``(logits, x leaf, parameter leaves, per-conv reports)``."""
    ei = torch.from_numpy(fx[f"{name}/edge_index"]).long()
    x, _, _, _ = gc.raw_data(c)
    if sd64 is None:
        sd64 = gc.perturbed(_product_model(c, fx, name).state_dict(), c)
    sd = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in sd64.items()}
    xo = torch.from_numpy(x).requires_grad_(True)
    if masks is None:
        masks = [torch.from_numpy(m) for m in gc.masks(c)] or None
    reports = []
    lo = orc.cegat_forward(sd, xo, ei, gc.n_convs(c), c["heads"], c["oheads"], masks, bn=c["norm"] == "bn", training=c["train"],
                           reports=reports)
    G = torch.from_numpy(gc.cotangent(c, lo.shape[0]))
    (lo * G).sum().backward()
    return lo, xo, sd, reports


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_oracle_equals_recorded_reference(name):
    c = gc.spec(name)
    fx = _fx(name)
    lo, xo, sd, _ = oracle_run(c, fx, name)
    gc.assert_result(lo, fx, name, "logits", rtol=2e-5, atol=2e-5)
    gc.assert_result(xo.grad, fx, name, "grad_x", rtol=2e-5, atol=2e-5)
    checked = 0
    for k, p in sd.items():
        if p.requires_grad and not k.endswith(("running_mean", "running_var")) and "lin_r" not in k:
            g = p.grad                                                      # (the restatement reads lin_l.weight alone: lin_r is its alias)
            gc.assert_result(g, fx, name, f"grad:{k}", rtol=2e-5, atol=2e-5 * max(1.0, float(g.abs().max())))
            checked += 1
    assert checked == 4 * gc.n_convs(c) + (2 * (gc.n_convs(c) - 1) if c["norm"] == "bn" else 0)


@pytest.mark.parametrize("name", sorted(gc.CASES))
def test_recorded_graph_has_the_quirks(name):
    """Pairs in one direction; the reference's V2V loops stop at max id + 1, GATConv's cover every vertex."""
    c = gc.spec(name)
    ei = torch.from_numpy(_fx(name)[f"{name}/edge_index"]).long()
    pairs = ei[:, ei[0] != ei[1]]
    assert bool((pairs[0] < pairs[1]).all())
    n = int(ei.max()) + 1
    assert n <= c["n_v"] - c["trailing"] and int((ei[0] == ei[1]).sum()) == n
    att = orc.attention_edges(ei, c["n_v"])
    assert int((att[0] == att[1]).sum()) == c["n_v"]
    deg = torch.bincount(att[1], minlength=c["n_v"])
    assert int(deg.min()) == 1 and bool((deg[n:] == 1).all())
    for v in c["interior"]:
        assert int(deg[v]) == 1


@pytest.mark.skipif(not __import__("oracle.ref_shim", fromlist=["x"]).available(), reason="needs the reference sources")
def test_fixtures_regenerate_byte_for_byte():
    import subprocess
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_cegat_fixtures.py"), "--check"], capture_output=True,
                         text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
