"""CPU: preprocessing and module surface of the HGNN / HCHA / HNHN baselines -- the degree scales computed from edge lists equal the
reference's dense-matrix formulas (restated in tests/baselines_oracle.py), the driver's preprocessing branch, the modules'
parameter layout, and train.build_model."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baselines_oracle as orc  # noqa: E402


def _edges(seed, n_v=60, n_e=25, isolated=0):
    rng = np.random.default_rng(seed)
    pairs = set()
    for e in range(n_e):
        for v in rng.choice(n_v - isolated, size=int(rng.integers(1, 7)), replace=False):
            pairs.add((int(v), e))
    return torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous(), n_v


@pytest.mark.parametrize("isolated", [0, 3])
@pytest.mark.parametrize("alpha,beta", [(-1.5, -0.5), (0.5, 1.0)])
def test_hnhn_norms_equal_dense_formulas(isolated, alpha, beta):
    from allset_amd.preprocessing import generate_norm_HNHN
    ei, n_v = _edges(1, isolated=isolated)
    data = SimpleNamespace(edge_index=ei + torch.tensor([[0], [n_v]]), n_x=[n_v])     # ids before the re-base, as train.py has them
    generate_norm_HNHN(None, data, SimpleNamespace(HNHN_alpha=alpha, HNHN_beta=beta))
    want = orc.hnhn_norms_dense(ei, n_v, alpha, beta)
    for k, v in want.items():
        got = getattr(data, k)
        assert got.dtype == torch.float32 and got.shape == (len(v),), k
        np.testing.assert_allclose(got.numpy(), v.astype(np.float32), rtol=1e-6, err_msg=k)
    if isolated and beta < 0:
        assert torch.isinf(data.D_v_beta[-isolated:]).all()          # 0 ** beta, as the reference's numpy computes it


@pytest.mark.parametrize("sym", [False, True])
def test_hcha_scales_equal_oracle(sym):
    from allset_amd.preprocessing import generate_norm_HCHA
    ei, n_v = _edges(2, isolated=2)
    data = SimpleNamespace(x=torch.zeros(n_v, 3), edge_index=ei)
    generate_norm_HCHA(data, sym)
    D, B = orc.hcha_scales(ei, n_v, sym)
    torch.testing.assert_close(data.HCHA_D.double(), D, rtol=1e-6, atol=0)
    torch.testing.assert_close(data.HCHA_B.double(), B, rtol=1e-6, atol=0)
    assert (data.HCHA_D[-2:] == 0).all()                             # 1 / 0 -> 0


def test_driver_preprocessing_branch():
    from allset_amd.train import build_parser, preprocess, synthetic_dataset
    for method, extra in (("HNHN", []), ("HCHA", []), ("HGNN", ["--HCHA_symdegnorm"])):
        args = build_parser().parse_args(["--method", method] + extra)
        data = preprocess(args, synthetic_dataset(n_v=300, n_e=120, seed=0))
        ei = data.edge_index
        assert int(ei[1].min()) == 0 and int(ei[0].max()) < 300
        assert torch.bincount(ei[0], minlength=300).min() >= 1            # self-loops: every vertex is in some hyperedge
        if method == "HNHN":
            M = int(ei[1].max()) + 1
            assert data.D_e_alpha.shape == (M,) and data.D_v_beta.shape == (300,)
            want = orc.hnhn_norms_dense(ei, 300, args.HNHN_alpha, args.HNHN_beta)
            np.testing.assert_allclose(data.D_e_beta_inv.numpy(), want["D_e_beta_inv"].astype(np.float32), rtol=1e-6)
        else:
            D, _ = orc.hcha_scales(ei, 300, args.HCHA_symdegnorm)
            torch.testing.assert_close(data.HCHA_D.double(), D, rtol=1e-6, atol=0)


# the reference's parameter names, shapes and dtypes (HypergraphConv.weight is [in, out]; HNHNConv holds two nn.Linear)
HCHA_L2 = [("convs.0.weight", (24, 32)), ("convs.0.bias", (32,)), ("convs.1.weight", (32, 5)), ("convs.1.bias", (5,))]
HNHN_L2 = [("convs.0.weight_v2e.weight", (32, 24)), ("convs.0.weight_v2e.bias", (32,)), ("convs.0.weight_e2v.weight", (32, 32)),
           ("convs.0.weight_e2v.bias", (32,)), ("convs.1.weight_v2e.weight", (32, 32)), ("convs.1.weight_v2e.bias", (32,)),
           ("convs.1.weight_e2v.weight", (5, 32)), ("convs.1.weight_e2v.bias", (5,))]


def _args(method, **kw):
    from allset_amd.train import build_parser
    a = build_parser().parse_args(["--method", method, "--MLP_hidden", "32"])
    a.num_features, a.num_classes = 24, 5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("method,L,want", [("HCHA", 2, HCHA_L2), ("HGNN", 1, HCHA_L2), ("HNHN", 2, HNHN_L2),
                                           ("HNHN", 1, [("convs.0.weight_v2e.weight", (32, 24)), ("convs.0.weight_v2e.bias", (32,)),
                                                        ("convs.0.weight_e2v.weight", (5, 32)), ("convs.0.weight_e2v.bias", (5,))])])
def test_build_model_state_dict_layout(method, L, want):
    from allset_amd.train import build_model
    model = build_model(_args(method, All_num_layers=L), None)
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == want
    assert all(v.dtype == torch.float32 for v in model.state_dict().values())


def test_hcha_init_and_refusals():
    from allset_amd.baselines import HypergraphConv
    conv = HypergraphConv(24, 32)
    assert torch.all(conv.bias == 0)
    bound = (6.0 / (24 + 32)) ** 0.5
    assert float(conv.weight.abs().max()) <= bound
    with pytest.raises(NotImplementedError):
        HypergraphConv(24, 32, use_attention=True)


@pytest.mark.parametrize("method", ["HyperGCN", "CEGCN", "CEGAT", "UniGCNII", "MLP"])
def test_out_of_scope_methods_still_raise(method):
    from allset_amd.train import build_model
    with pytest.raises(ValueError):
        build_model(_args(method), None)


def test_hgnn_symdegnorm_flag_is_live():
    from allset_amd.train import build_model
    assert build_model(_args("HGNN", HCHA_symdegnorm=True), None).convs[0].symdegnorm is True
    assert build_model(_args("HCHA"), None).convs[0].symdegnorm is False


def test_oracle_conv_matches_dense_restatement():
    ei, n_v = _edges(4)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n_v, 6, generator=g, dtype=torch.float64)
    w = torch.randn(6, 4, generator=g, dtype=torch.float64)
    b = torch.randn(4, generator=g, dtype=torch.float64)
    for sym in (False, True):
        torch.testing.assert_close(orc.hypergraph_conv(x, ei, w, b, sym), orc.dense_hcha_conv(x, ei, w, b, sym))
