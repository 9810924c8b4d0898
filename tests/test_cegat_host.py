"""CPU: the CEGAT baseline's host-side surface -- GATConv's torch_geometric 1.6.3 parameter layout and initialisation order, the
arguments CEGAT refuses (the two families on which the reference's module fails at its first forward), train.build_model's checks,
and the float64 restatement tests/cegat_oracle.py against its dense form (masked softmax over A + I) with the quirks the product
must reproduce."""
import math
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cegat_oracle as orc  # noqa: E402


def _args(**kw):
    from allset_amd.train import build_parser
    a = build_parser().parse_args(["--method", "CEGAT"])
    a.num_features, a.num_classes = 12, 4
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _data(**kw):
    d = dict(clique_expansion=True, edge_index=torch.tensor([[0, 1], [1, 2]]))
    d.update(kw)
    return SimpleNamespace(**d)


def test_gatconv_parameter_surface_is_torch_geometric_1_6_3():
    from allset_amd.baselines import GATConv
    conv = GATConv(12, 5, heads=3)
    assert conv.lin_r is conv.lin_l
    assert [(k, tuple(v.shape)) for k, v in conv.state_dict().items()] == [
        ("att_l", (1, 3, 5)), ("att_r", (1, 3, 5)), ("bias", (15,)), ("lin_l.weight", (15, 12)), ("lin_r.weight", (15, 12))]
    assert [k for k, _ in conv.named_parameters()] == ["att_l", "att_r", "bias", "lin_l.weight"]
    assert tuple(GATConv(12, 5, heads=3, concat=False).bias.shape) == (5,)
    assert GATConv(12, 5, bias=False).bias is None
    assert float(conv.bias.detach().abs().max()) == 0.0
    assert float(conv.att_l.detach().abs().max()) <= math.sqrt(6.0 / (3 + 5))
    assert float(conv.lin_l.weight.detach().abs().max()) <= math.sqrt(6.0 / 27)


def test_gatconv_initialisation_draws_in_the_order_of_1_6_3():
    """Linear's own init, then glorot on lin_l.weight, on lin_r.weight (the same tensor: a second draw), on att_l, on att_r."""
    from allset_amd.baselines import GATConv
    torch.manual_seed(11)
    conv = GATConv(6, 4, heads=2)
    torch.manual_seed(11)
    torch.nn.Linear(6, 8, bias=False)
    a = math.sqrt(6.0 / (6 + 8))
    torch.empty(8, 6).uniform_(-a, a)
    w = torch.empty(8, 6).uniform_(-a, a)
    b = math.sqrt(6.0 / (2 + 4))
    al = torch.empty(1, 2, 4).uniform_(-b, b)
    ar = torch.empty(1, 2, 4).uniform_(-b, b)
    assert torch.equal(conv.lin_l.weight, w) and torch.equal(conv.att_l, al) and torch.equal(conv.att_r, ar)


def test_gatconv_refuses_what_is_not_built():
    from allset_amd.baselines import GATConv
    with pytest.raises(NotImplementedError, match="attention"):
        GATConv(4, 4, dropout=0.5)
    with pytest.raises(NotImplementedError, match="bipartite"):
        GATConv((4, 6), 4)
    with pytest.raises(NotImplementedError, match="bipartite"):
        GATConv(4, 4)((torch.zeros(3, 4), torch.zeros(3, 4)), torch.zeros(2, 0, dtype=torch.int64))


def test_cegat_structure_follows_the_reference():
    from allset_amd.baselines import CEGAT, GATConv
    m = CEGAT(12, 16, 4, 1, heads=4, output_heads=2, dropout=0.5, Normalization='ln')
    assert [(c.in_channels, c.out_channels, c.heads, c.concat) for c in m.convs] == [(12, 16, 4, True), (64, 4, 2, False)]
    assert all(isinstance(n, torch.nn.Identity) for n in m.normalizations) and len(m.normalizations) == 1
    m = CEGAT(12, 16, 4, 3, heads=1, output_heads=1, dropout=0.5, Normalization='bn')
    assert [(c.in_channels, c.out_channels, c.heads, c.concat) for c in m.convs] == [(12, 16, 1, True), (16, 16, 1, True), (16, 4, 1, False)]
    assert all(isinstance(n, torch.nn.BatchNorm1d) for n in m.normalizations) and len(m.normalizations) == 2
    assert all(isinstance(c, GATConv) for c in m.convs)


def test_cegat_refuses_the_arguments_the_reference_fails_on():
    from allset_amd.baselines import CEGAT
    with pytest.raises(ValueError, match="middle"):
        CEGAT(12, 16, 4, 3, heads=2, output_heads=1, dropout=0.5, Normalization='ln')
    with pytest.raises(ValueError, match="BatchNorm1d"):
        CEGAT(12, 16, 4, 2, heads=2, output_heads=1, dropout=0.5, Normalization='bn')
    CEGAT(12, 16, 4, 2, heads=2, output_heads=3, dropout=0.5, Normalization='ln')
    CEGAT(12, 16, 4, 3, heads=1, output_heads=3, dropout=0.5, Normalization='bn')


def test_build_model_builds_cegat_on_flagged_data_with_an_edge_list():
    from allset_amd.baselines import CEGAT
    from allset_amd.train import CE_METHODS, build_model
    assert CE_METHODS == ('CEGCN', 'CEGAT')
    m = build_model(_args(heads=4, output_heads=2, MLP_hidden=16, All_num_layers=2), _data())
    assert isinstance(m, CEGAT) and m.convs[0].heads == 4 and m.convs[-1].heads == 2 and not m.convs[-1].concat
    for bad in (None, SimpleNamespace(clique_expansion=True), _data(clique_expansion=False), _data(edge_index=torch.zeros(3, 4, dtype=torch.int64)),
                _data(edge_index=torch.zeros(2, 4)), _data(edge_index=[[0], [1]])):
        with pytest.raises(ValueError, match="train.preprocess"):
            build_model(_args(), bad)
    with pytest.raises(ValueError, match="middle"):
        build_model(_args(heads=2, All_num_layers=3), _data())
    with pytest.raises(ValueError, match="BatchNorm1d"):
        build_model(_args(heads=2, normalization='bn'), _data())


def test_no_cpu_path():
    from allset_amd._lib import AllSetHipError
    from allset_amd.baselines import CEGAT
    m = CEGAT(12, 16, 4, 2, heads=1, output_heads=1, dropout=0.5, Normalization='ln')
    with pytest.raises(AllSetHipError):
        m(SimpleNamespace(x=torch.zeros(3, 12), edge_index=torch.tensor([[0, 1], [1, 2]])))


# ---- the restatement against its dense form, and the quirks ----------------------------------------------------------------------
def _conv_sd(F, C, H, concat, g):
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    return {"c.lin_l.weight": r(H * C, F), "c.att_l": r(1, H, C), "c.att_r": r(1, H, C), "c.bias": r(H * C if concat else C)}


@pytest.mark.parametrize("H,concat", [(1, True), (4, True), (2, False)])
def test_restatement_equals_dense_masked_softmax(H, concat):
    g = torch.Generator().manual_seed(H)
    n = 40
    ei = torch.unique(torch.randint(0, n - 3, (2, 150), generator=g), dim=1)
    ei = ei[:, ei[0] < ei[1]]                                               # one direction, as ConstructV2V leaves the pairs
    ei = torch.cat([ei, torch.tensor([[2, 9], [2, 9]])], dim=1)             # loops already present: dropped, then re-added once
    x = torch.randn(n, 7, generator=g, dtype=torch.float64)
    sd = _conv_sd(7, 5, H, concat, g)
    rep = {}
    got = orc.gat_conv(x, ei, sd, "c.", H, concat, report=rep)
    torch.testing.assert_close(got, orc.dense_gat(x, ei, sd, "c.", H, concat), rtol=1e-12, atol=1e-12)
    xw = x @ sd["c.lin_l.weight"].t()
    for v in (n - 1, n - 2, int(ei[0].min())):                              # trailing isolated ids; an id that hears from nobody
        own = xw[v].view(H, 5)                                              # (pairs i < j: the smallest id has no in-edge)
        torch.testing.assert_close(got[v], (own.reshape(-1) if concat else own.mean(0)) + sd["c.bias"], rtol=1e-12, atol=1e-12)
    assert rep["p"].shape[0] == int((ei[0] != ei[1]).sum()) + n             # every vertex has exactly one loop


def test_restatement_ignores_edge_multiplicity_and_size_one_hyperedges():
    import ce_oracle as ce
    v2e = torch.tensor([[0, 1, 0, 1, 2, 3, 0, 1], [10, 10, 11, 11, 11, 12, 13, 13]])       # pair (0, 1) three times; 12 has one member
    pairs, mult = ce.clique_expansion(v2e)
    assert pairs.t().tolist() == [[0, 1], [0, 2], [1, 2]] and mult.tolist() == [3.0, 1.0, 1.0]
    att = orc.attention_edges(pairs, 5)
    assert att.t().tolist() == [[0, 1], [0, 2], [1, 2], [0, 0], [1, 1], [2, 2], [3, 3], [4, 4]]
