"""CPU: the clique-expansion baseline CEGCN's module surface and its float64 restatement (tests/ce_oracle.py) -- the restatement
against the dense ``D^-1/2 (A + I') D^-1/2 X W + b`` with the reference's quirks (shared pairs, size-1 hyperedges, interior and
trailing isolated vertices), the parameter layout and initialisation, and train.build_model's refusal of data that has not been
through the V2V branch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_oracle as orc  # noqa: E402


def _hyperedges(seed, n_v=40, n_e=18, trailing=3, interior=(7,)):
    """(vertex, hyperedge) incidences: sizes 1..6, one pair shared by three hyperedges, no member among the ``interior`` ids
    and the last ``trailing`` vertices."""
    rng = np.random.default_rng(seed)
    pool = np.array([v for v in range(n_v - trailing) if v not in interior])
    pairs = set()
    for e in range(n_e):
        k = 1 if e in (2, 5) else int(rng.integers(2, 7))
        for v in rng.choice(pool, size=k, replace=False):
            pairs.add((int(v), e))
    for e in (n_e, n_e + 1, n_e + 2):                       # the pair (0, 1) in three more hyperedges
        pairs |= {(0, e), (1, e)}
    return torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous(), n_v


def test_oracle_equals_dense_form_with_quirks():
    ei, n_v = _hyperedges(0)
    pairs, mult = orc.clique_expansion(ei)
    assert bool((pairs[0] < pairs[1]).all())                                   # one direction only
    k = ((pairs[0] == 0) & (pairs[1] == 1)).nonzero()
    assert float(mult[k]) >= 3.0                                               # multiplicity of a shared pair
    n = int(pairs.max()) + 1
    assert n < n_v                                                             # trailing isolated ids: no loop
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n_v, 5, generator=g, dtype=torch.float64)
    w = torch.randn(5, 3, generator=g, dtype=torch.float64)
    b = torch.randn(3, generator=g, dtype=torch.float64)
    gei, gw = orc.gcn_norm(pairs, mult)
    got = orc.gcn_conv(x, gei, gw, w, b)
    torch.testing.assert_close(got, orc.dense_gcn(x, pairs, mult, w, b), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(got[n:], b.expand(n_v - n, 3))                  # trailing vertices: the bias alone
    torch.testing.assert_close(got[7], (x[7] @ w) + b)                         # interior isolated vertex: its own loop, weight 1


def _args(**kw):
    from allset_amd.train import build_parser
    a = build_parser().parse_args(["--method", "CEGCN", "--MLP_hidden", "32"])
    a.num_features, a.num_classes = 24, 5
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _ce_data():
    from types import SimpleNamespace
    return SimpleNamespace(clique_expansion=True)


@pytest.mark.parametrize("L,norm,want", [
    (1, "ln", [("convs.0.weight", (24, 32)), ("convs.0.bias", (32,)), ("convs.1.weight", (32, 5)), ("convs.1.bias", (5,))]),
    (3, "ln", [("convs.0.weight", (24, 32)), ("convs.0.bias", (32,)), ("convs.1.weight", (32, 32)), ("convs.1.bias", (32,)),
               ("convs.2.weight", (32, 5)), ("convs.2.bias", (5,))]),
    (2, "bn", [("convs.0.weight", (24, 32)), ("convs.0.bias", (32,)), ("convs.1.weight", (32, 5)), ("convs.1.bias", (5,)),
               ("normalizations.0.weight", (32,)), ("normalizations.0.bias", (32,)), ("normalizations.0.running_mean", (32,)),
               ("normalizations.0.running_var", (32,)), ("normalizations.0.num_batches_tracked", ())]),
])
def test_cegcn_state_dict_layout(L, norm, want):
    from allset_amd.train import build_model
    model = build_model(_args(All_num_layers=L, normalization=norm), _ce_data())
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == want
    assert len(model.normalizations) == len(model.convs) - 1
    kinds = {type(m).__name__ for m in model.normalizations}
    assert kinds == ({"BatchNorm1d"} if norm == "bn" else {"Identity"})


@pytest.mark.parametrize("L", [1, 2, 3])
def test_cegcn_initial_parameters_under_manual_seed(L):
    """GCNConv draws glorot U(-a, a) for its [in, out] weight at construction, conv by conv; biases are zeros."""
    from allset_amd.baselines import CEGCN
    torch.manual_seed(7)
    model = CEGCN(24, 32, 5, L, 0.5, Normalization="ln")
    torch.manual_seed(7)
    dims = [(24, 32)] + [(32, 32)] * (L - 2) + [(32, 5)]
    for i, (fi, fo) in enumerate(dims):
        a = (6.0 / (fi + fo)) ** 0.5
        want = torch.empty(fi, fo).uniform_(-a, a)
        assert torch.equal(model.convs[i].weight.detach(), want), i
        assert torch.all(model.convs[i].bias == 0)


def test_build_model_requires_the_v2v_branch():
    from types import SimpleNamespace
    from allset_amd.train import build_model
    for data in (None, SimpleNamespace(edge_index=torch.zeros((2, 3), dtype=torch.int64))):
        with pytest.raises(ValueError, match="clique expansion"):
            build_model(_args(), data)
    with pytest.raises(ValueError):
        build_model(_args(method="CEGAT"), _ce_data())                       # not built


def test_gcnconv_refuses_normalize_true():
    from allset_amd.baselines import GCNConv
    with pytest.raises(NotImplementedError):
        GCNConv(4, 4)
    conv = GCNConv(24, 32, normalize=False)
    assert conv.weight.shape == (24, 32) and torch.all(conv.bias == 0)
