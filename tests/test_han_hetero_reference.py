"""CPU: the heterogeneous HAN against what the REFERENCE computed (tests/golden/baselines_han_hetero.npz, recorded by
tools/gen_han_hetero_fixtures.py from the reference's own DGL_HAN/model_hetero.py classes with stand-ins for
``dgl.metapath_reachable_graph`` and ``dgl.nn.pytorch.GATConv``).  Checked here: the product's initial parameters and ``state_dict``
layout equal the reference's draw under ``torch.manual_seed``; the fixture's recorded inputs are the ones tests/han_hetero_cases.py
rebuilds; the functional float64 restatement of tests/han_hetero_oracle.py reproduces logits, d/dx and every parameter gradient to 2e-5
(the level of tests/test_han_reference.py); every case keeps 1e-5 away from the leaky-relu kink and does contain rows without an
incoming edge; the scipy reachability against a dense numpy product.  Where the reference is importable the fixtures are regenerated and
compared byte for byte."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_hetero_cases as hc  # noqa: E402
import han_hetero_oracle as horc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=2e-5, atol=2e-5)


def product_model(c):
    from allset_amd.han_hetero import HAN
    torch.manual_seed(c["seed"])
    return HAN(meta_paths=hc.META_PATHS, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=hc.DROPOUT)


def oracle_run(c, masks="case"):
    x, edges, num_nodes = hc.raw_data(c)
    g = horc.TypedGraph(edges, num_nodes)
    graphs = [tuple(torch.from_numpy(a) for a in horc.reachable_edges(g, mp)) for mp in hc.META_PATHS]
    n = num_nodes["paper"]
    sd64 = hc.perturb(product_model(c).state_dict(), c)
    if isinstance(masks, str):
        masks = hc.masks(c, [s.numel() for s, _ in graphs])
        if masks is not None:
            masks = [[tuple(torch.from_numpy(m) for m in pair) for pair in layer] for layer in masks]
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    xo = torch.from_numpy(x).clone().requires_grad_(True)
    report = []
    out = horc.han_forward(sd, graphs, n, xo, len(c["heads"]), masks, report)
    (out * torch.from_numpy(hc.cotangent(c, n))).sum().backward()
    return out, xo, sd, min(report), graphs


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    c = hc.spec(name)
    fx = hc.load(hc.FILE)
    model = product_model(c)
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert hc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
    keys = list(model.state_dict())
    assert keys[:4] == ["layers.0.gat_layers.0.attn_l", "layers.0.gat_layers.0.attn_r", "layers.0.gat_layers.0.bias",
                        "layers.0.gat_layers.0.fc.weight"]
    assert model.layers[0].meta_paths == [("pa", "ap"), ("pf", "fp")]
    assert all(conv._allow_zero_in_degree for layer in model.layers for conv in layer.gat_layers)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_recorded_inputs_are_the_cases(name):
    c = hc.spec(name)
    fx = hc.load(hc.FILE)
    x, edges, _ = hc.raw_data(c)
    assert np.array_equal(fx[f"{name}/x"], x)
    for (s, e, d), (src, dst) in edges.items():
        assert np.array_equal(fx[f"{name}/edges:{s}|{e}|{d}"], np.stack([src, dst]))
    sd = hc.perturb(product_model(c).state_dict(), c)
    for k, v in sd.items():
        assert np.array_equal(fx[f"{name}/param:{k}"], v.numpy()), k


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_restatement_equals_reference(name):
    c = hc.spec(name)
    fx = hc.load(hc.FILE)
    out, xo, sd, margin, graphs = oracle_run(c)
    print(f"{name}: kink margin {margin:.3e} (recorded {float(fx[name + '/margin']):.3e})")
    assert margin > hc.KINK_MARGIN and float(fx[f"{name}/margin"]) > hc.KINK_MARGIN
    hc.assert_result(out, fx, name, "out", **TOL)
    hc.assert_result(xo.grad, fx, name, "grad_x", **TOL)
    for k, v in sd.items():
        hc.assert_result(v.grad, fx, name, f"grad:{k}", **TOL)


def test_cases_cover_what_the_issue_lists():
    specs = [hc.spec(n) for n in hc.CASES]
    assert any(c["heads"] == [1] for c in specs) and any(max(c["heads"]) > 1 for c in specs) and any(len(c["heads"]) == 2 for c in specs)
    assert any(c["train"] for c in specs) and any(not c["train"] for c in specs)
    for c in specs:
        assert (c["n_p"], c["n_a"], c["n_f"]) == (40, 25, 4)
        x, edges, num_nodes = hc.raw_data(c)
        g = horc.TypedGraph(edges, num_nodes)
        (ps, pd), (fs, fd) = (horc.reachable_edges(g, mp) for mp in hc.META_PATHS)
        assert (np.bincount(pd, minlength=40) == 0).sum() == c["orphans"] > 0               # PAP: targets without an incoming edge
        assert (np.bincount(fd, minlength=40) == 0).sum() == 0 and np.bincount(fd).max() > 10   # PFP: none, and a hub field
        assert np.unique(ps * 40 + pd).size == ps.size                                       # one edge per pair despite duplicates
        pa = edges[hc.RELATIONS[0]]
        assert pa[0].size > np.unique(pa[0] * 25 + pa[1]).size                               # duplicate input pairs


def test_scipy_reachability_equals_a_dense_product():
    c = hc.spec("hetero_h1")
    _, edges, num_nodes = hc.raw_data(c)
    g = horc.TypedGraph(edges, num_nodes)
    dense = {}
    for (s, e, d), (src, dst) in edges.items():
        m = np.zeros((num_nodes[s], num_nodes[d]))
        m[src, dst] = 1.0
        dense[e] = m
    for mp in (["pa", "ap"], ["pf", "fp"], ["pa"], ["ap", "pf"], ["fp", "pa", "ap"], ["pa", "ap", "pf", "fp"]):
        want = dense[mp[0]]
        for e in mp[1:]:
            want = want @ dense[e]
        r, cc = np.nonzero(want > 0)
        src, dst = horc.reachable_edges(g, mp)
        assert np.array_equal(src, r) and np.array_equal(dst, cc), mp


def test_empty_row_rule_of_the_restatement():
    """A target without an incoming edge: elu(bias) forward; d/dx, d/del, d/der get nothing from it, d/dbias gets gy * elu'(bias)."""
    g = torch.Generator().manual_seed(0)
    n, H, C = 6, 2, 3
    src, dst = torch.tensor([0, 1, 2, 4]), torch.tensor([1, 1, 0, 0])                        # rows 2..5 are empty
    fs, el, er, b = (torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True) for s in ((n, H * C), (n, H), (n, H), (H * C,)))
    out = horc.gat_hop(src, dst, n, fs, el, er, b)
    assert torch.equal(out[2:].detach(), F.elu(b.detach()).expand(4, -1))
    out[2:].sum().backward()
    assert float(fs.grad.abs().max()) == 0 and float(el.grad.abs().max()) == 0 and float(er.grad.abs().max()) == 0
    torch.testing.assert_close(b.grad, 4 * torch.where(b.detach() > 0, torch.ones_like(b), b.detach().exp()))
    assert horc.gat_hop(src[:0], dst[:0], n, fs, el, er, b).shape == (n, H * C)


def test_explicit_dropout_factors_matter():
    c = hc.spec("hetero_h2_train")
    a = oracle_run(c)[0]
    b = oracle_run(c, masks=None)[0]
    assert float((a - b).detach().abs().max()) > 1e-2


def test_fixtures_regenerate_byte_for_byte():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_han_hetero_fixtures as gen
    if not gen.available():
        pytest.skip("the reference's sources are not on this machine")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_han_hetero_fixtures.py"), "--check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
