"""CPU: the UniGCNII baseline's host-side surface -- the preprocessing (``ConstructH_pairs`` / ``generate_norm_UniGNN``) against the
dense ``ConstructH`` formulas of the float64 restatement tests/unigcnii_oracle.py, with a repeated incidence, isolated vertices and
the inf -> 1 rule; the driver's ``preprocess`` branch; ``build_model``'s refusal of data that has not been through it; the module
layout; the two parameter groups and their weight decays; the folded identity-mapping weight."""
import math
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unigcnii_cases as uc  # noqa: E402
import unigcnii_oracle as orc  # noqa: E402


def _v2e():
    """Hyperedge ids 100.. with a gap (104 never occurs), vertex 3 (interior) and 8, 9 (trailing) in no hyperedge, (1, 102) twice."""
    rows = [(0, 100), (1, 100), (2, 100), (1, 102), (4, 102), (1, 102), (5, 103), (6, 105), (7, 105), (0, 105), (2, 101)]
    return torch.tensor(rows, dtype=torch.int64).t().contiguous(), 10


def test_pairs_and_scales_equal_the_dense_formulas():
    from allset_amd.preprocessing import ConstructH_pairs, generate_norm_UniGNN
    ei, n = _v2e()
    data = ConstructH_pairs(SimpleNamespace(x=torch.zeros(n, 3), edge_index=ei[:, torch.randperm(ei.shape[1])]))
    H = orc.dense_incidence(ei, n)
    V, E = orc.pairs(H)
    assert data.UniGNN_sizes == (n, 5) and data.edge_index.dtype == torch.int64
    assert torch.equal(data.edge_index, torch.stack([V, E]))                       # de-duplicated, renumbered, sorted by (v, e)
    assert data.edge_index.shape[1] == ei.shape[1] - 1
    args = SimpleNamespace()
    degV, degE, scaleE = generate_norm_UniGNN(data, args)
    assert args.UniGNN_degV is degV and args.UniGNN_degE is degE
    assert degV.shape == (n, 1) and degE.shape == (5, 1) and degV.dtype == degE.dtype == torch.float32
    wV, wE = orc.degrees(H)
    torch.testing.assert_close(degV.double(), wV, rtol=1e-6, atol=0)
    torch.testing.assert_close(degE.double(), wE, rtol=1e-6, atol=0)
    for v in (3, 8, 9):
        assert float(degV[v]) == 1.0                                               # inf -> 1
    assert float(degV[1]) == pytest.approx(2 ** -0.5)                              # the repeated pair counts once
    torch.testing.assert_close(scaleE.double(), wE.view(-1) / H.sum(0), rtol=1e-6, atol=0)
    assert data.UniGNN_scaleE is scaleE


def test_pairs_refuse_bad_input():
    from allset_amd.preprocessing import ConstructH_pairs, generate_norm_UniGNN
    ei, n = _v2e()
    with pytest.raises(ValueError, match="vertex ids"):
        ConstructH_pairs(SimpleNamespace(x=torch.zeros(5, 3), edge_index=ei))
    with pytest.raises(ValueError, match="empty"):
        ConstructH_pairs(SimpleNamespace(x=torch.zeros(5, 3), edge_index=torch.zeros((2, 0), dtype=torch.int64)))
    with pytest.raises(ValueError, match="ConstructH_pairs"):
        generate_norm_UniGNN(SimpleNamespace(x=torch.zeros(n, 3), edge_index=ei), SimpleNamespace())


def _preprocessed(name):
    from allset_amd.train import HypergraphData, build_parser, preprocess
    c = uc.spec(name)
    x, block, n_v, n_e = uc.raw_data(c)
    argv = ["--method", "UniGCNII"] + ([] if c["self_loops"] else ["--add_self_loop"])
    args = build_parser().parse_args(argv)
    assert args.add_self_loop == c["self_loops"]
    data = preprocess(args, HypergraphData(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(block), n_x=[n_v],
                                           num_hyperedges=[n_e]))
    return c, args, data, block


@pytest.mark.parametrize("name", ["uni_L2_h1", "uni_L2_noself"])
def test_driver_preprocess_branch(name):
    """train.preprocess against the dense formulas on the raw V->E half (+ one singleton hyperedge per vertex that is not already alone
    in one, with self-loops), and against the pairs and scales the REFERENCE recorded."""
    c, args, data, block = _preprocessed(name)
    n_v = c["n_v"]
    v2e = torch.from_numpy(block[:, block[0] < n_v])
    if c["self_loops"]:
        sizes = torch.bincount(v2e[1])
        alone = set(v2e[0][sizes[v2e[1]] == 1].tolist())
        new_v = [v for v in range(n_v) if v not in alone]
        new_e = int(v2e[1].max()) + 1 + torch.arange(len(new_v))
        v2e = torch.cat([v2e, torch.stack([torch.tensor(new_v), new_e])], dim=1)
    H = orc.dense_incidence(v2e, n_v)
    V, E = orc.pairs(H)
    assert torch.equal(data.edge_index, torch.stack([V, E])) and data.UniGNN_sizes == tuple(H.shape)
    wV, wE = orc.degrees(H)
    torch.testing.assert_close(args.UniGNN_degV.double(), wV, rtol=1e-6, atol=0)
    torch.testing.assert_close(args.UniGNN_degE.double(), wE, rtol=1e-6, atol=0)
    if not c["self_loops"]:
        iso = [v for v in range(n_v) if float(H[v].sum()) == 0]
        assert len(iso) >= 6 and min(iso) < n_v - c["trailing"]                    # interior and trailing isolated vertices
        assert all(float(args.UniGNN_degV[v]) == 1.0 for v in iso)
        assert int((block[0] < n_v).sum()) == V.numel() + 1                        # the repeated incidence collapsed
    fx = uc.load("baselines_unigcnii")
    np.testing.assert_array_equal(data.edge_index.numpy(), fx[f"{name}/pairs"].astype(np.int64))
    np.testing.assert_allclose(args.UniGNN_degV.numpy(), fx[f"{name}/degV"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(args.UniGNN_degE.numpy(), fx[f"{name}/degE"], rtol=1e-6, atol=0)


def test_build_model_needs_preprocessed_data():
    from allset_amd.baselines import UniGCNII
    from allset_amd.train import build_model, build_parser
    c, args, data, _ = _preprocessed("uni_L2_h1")
    args.num_features, args.num_classes = c["F"], c["C"]
    assert isinstance(build_model(args, data), UniGCNII)
    with pytest.raises(ValueError, match="preprocess"):
        build_model(args, None)
    with pytest.raises(ValueError, match="preprocess"):
        build_model(args, SimpleNamespace(edge_index=data.edge_index))             # pairs that never saw ConstructH_pairs
    fresh = build_parser().parse_args(["--method", "UniGCNII"])                     # UniGNN_degV / _degE still the parser's 0
    fresh.num_features, fresh.num_classes = c["F"], c["C"]
    with pytest.raises(ValueError, match="preprocess"):
        build_model(fresh, data)
    for method in ("HyperGCN", "MLP"):
        args.method = method
        with pytest.raises(ValueError, match="out of scope"):
            build_model(args, data)


def test_module_layout_and_parameter_groups():
    from allset_amd.baselines import UniGCNII, UniGCNIIConv
    from allset_amd.train import make_optimizer
    args = SimpleNamespace(method="UniGCNII", UniGNN_degV=torch.ones(4, 1), UniGNN_degE=torch.ones(2, 1), UniGNN_use_norm=False,
                           lr=0.5, wd=0.25)
    V, E = torch.tensor([0, 1, 2, 3]), torch.tensor([0, 0, 1, 1])
    model = UniGCNII(args, nfeat=6, nhid=4, nclass=3, nlayer=3, nhead=2, V=V, E=E)
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [
        ("convs.0.weight", (8, 6)), ("convs.0.bias", (8,)), ("convs.1.W.weight", (8, 8)), ("convs.2.W.weight", (8, 8)),
        ("convs.3.W.weight", (8, 8)), ("convs.4.weight", (3, 8)), ("convs.4.bias", (3,))]
    assert all(isinstance(m, UniGCNIIConv) for m in model.convs[1:-1]) and model.V is V and model.E is E
    assert model.dropout.p == 0.2
    names = {id(p): k for k, p in model.named_parameters()}
    assert [names[id(p)] for p in model.reg_params] == ["convs.1.W.weight", "convs.2.W.weight", "convs.3.W.weight"]
    assert [names[id(p)] for p in model.non_reg_params] == ["convs.0.weight", "convs.0.bias", "convs.4.weight", "convs.4.bias"]
    opt = make_optimizer(args, model)
    assert [(g["weight_decay"], g["lr"]) for g in opt.param_groups] == [(0.01, 0.01), (5e-4, 0.01)]      # --lr / --wd ignored
    assert all(a is b for a, b in zip(opt.param_groups[0]["params"], model.reg_params))
    assert all(a is b for a, b in zip(opt.param_groups[1]["params"], model.non_reg_params))
    args.method = "HCHA"
    other = make_optimizer(args, model)
    assert len(other.param_groups) == 1 and other.param_groups[0]["lr"] == 0.5 and other.param_groups[0]["weight_decay"] == 0.25
    with pytest.raises(Exception, match="device"):
        model(SimpleNamespace(x=torch.zeros(4, 6)))                                # no CPU path


def test_reset_parameters_is_each_modules_own():
    from allset_amd.baselines import UniGCNII
    args = SimpleNamespace(UniGNN_degV=torch.ones(4, 1), UniGNN_degE=torch.ones(2, 1), UniGNN_use_norm=False)
    torch.manual_seed(5)
    model = UniGCNII(args, 6, 4, 3, 2, 1, torch.tensor([0, 1]), torch.tensor([0, 1]))
    first = {k: v.clone() for k, v in model.state_dict().items()}
    torch.manual_seed(5)
    want = [torch.nn.Linear(6, 4), torch.nn.Linear(4, 4, bias=False), torch.nn.Linear(4, 4, bias=False), torch.nn.Linear(4, 3)]
    assert torch.equal(first["convs.0.weight"], want[0].weight) and torch.equal(first["convs.2.W.weight"], want[2].weight)
    assert torch.equal(first["convs.3.bias"], want[3].bias)
    torch.manual_seed(5)
    model.reset_parameters()
    for k, v in model.state_dict().items():
        assert torch.equal(v, first[k]), k


def test_folded_weight_is_the_identity_mapping_step():
    from allset_amd.baselines import UniGCNIIConv
    conv = UniGCNIIConv(SimpleNamespace(), 6, 6).double()
    beta = math.log(0.5 / 2 + 1)
    xi = torch.randn(9, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    w = conv.folded_weight(beta)
    torch.testing.assert_close(xi @ w.t(), (1 - beta) * xi + beta * conv.W(xi), rtol=1e-12, atol=1e-12)
    (xi @ w.t()).sum().backward()
    torch.testing.assert_close(conv.W.weight.grad, beta * xi.sum(0).expand(6, 6), rtol=1e-12, atol=1e-12)
    with pytest.raises(ValueError, match="square"):
        UniGCNIIConv(SimpleNamespace(), 6, 5).folded_weight(beta)
