"""Host-side contract of the hypergraph attention path: the layer's parameters against the reference layer's (keys, shapes and the
checksum of the initial values the fixture recorded), the refusals, the model wiring and the driver's flags.  No GPU."""
import os
import sys
from types import SimpleNamespace

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hcha_attn_cases as hc  # noqa: E402


@pytest.fixture(scope="module")
def fx():
    return hc.load(hc.FILE)


@pytest.mark.parametrize("name", sorted(hc.CASES))
def test_state_dict_equals_reference_layer(fx, name):
    from allset_amd.baselines import HypergraphAttentionConv
    c = hc.spec(name)
    torch.manual_seed(c["seed"])
    conv = HypergraphAttentionConv(hc.F_IN, c["out"], heads=c["heads"], concat=c["concat"],
                          dropout=hc.ATTN_DROP if c["train"] else 0)
    sd = conv.state_dict()
    keys = "|".join(f"{k}:{'x'.join(str(s) for s in v.shape)}" for k, v in sd.items())
    assert keys == bytes(fx[f"{name}/keys"]).decode()
    assert hc.checksum(sd) == bytes(fx[f"{name}/chk"]).decode()
    H, C = c["heads"], c["out"]
    assert tuple(sd["weight"].shape) == (hc.F_IN, H * C) and tuple(sd["att"].shape) == (1, H, 2 * C)
    assert tuple(sd["bias"].shape) == ((H * C,) if c["concat"] else (C,))


def _ei(n_v, n_e):
    return torch.stack([torch.arange(n_e) % n_v, torch.arange(n_e)])


def test_refusals():
    from allset_amd.baselines import HypergraphAttentionConv, HypergraphConv
    with pytest.raises(ValueError, match="symdegnorm"):
        HypergraphAttentionConv(6, 4, symdegnorm=True)
    with pytest.raises(NotImplementedError, match="HypergraphAttentionConv"):       # the plain class keeps its refusal and names the way
        HypergraphConv(6, 4, use_attention=True)
    conv = HypergraphAttentionConv(6, 4, heads=2)
    x = torch.randn(5, 6)
    with pytest.raises(ValueError, match="n_e <= n_v"):
        conv(x, _ei(5, 7))                                              # reference mode: more hyperedges than vertices
    with pytest.raises(ValueError, match="hyperedge_attr"):
        conv(x, _ei(5, 7), hyperedge_attr=torch.randn(7, 5))            # wrong width
    with pytest.raises(ValueError, match="hyperedge_attr"):
        conv(x, _ei(5, 7), hyperedge_attr=torch.randn(6, 6))            # wrong row count
    with pytest.raises(ValueError, match="hyperedge_attr"):
        conv(x, _ei(5, 7), hyperedge_attr="max")
    with pytest.raises(ValueError, match="hyperedge_weight"):
        conv(x, _ei(5, 4), hyperedge_weight=torch.ones(5))
    with pytest.raises(ValueError, match="hyperedge_weight"):
        HypergraphConv(6, 4)(x, _ei(5, 4), hyperedge_weight=torch.ones(4, 1))


def test_weighted_scales():
    from allset_amd.preprocessing import generate_norm_HCHA
    ei = torch.tensor([[0, 1, 1, 2, 4], [0, 0, 1, 1, 2]])
    w = torch.tensor([0.5, 1.5, 2.0])
    d = generate_norm_HCHA(SimpleNamespace(x=torch.zeros(6, 1), edge_index=ei), False, w)
    torch.testing.assert_close(d.HCHA_D, torch.tensor([2.0, 0.5, 1 / 1.5, 0.0, 0.5, 0.0]))
    torch.testing.assert_close(d.HCHA_B, torch.tensor([0.5, 0.5, 1.0]))
    plain = generate_norm_HCHA(SimpleNamespace(x=torch.zeros(6, 1), edge_index=ei), False)
    ones = generate_norm_HCHA(SimpleNamespace(x=torch.zeros(6, 1), edge_index=ei), False, torch.ones(3))
    assert torch.equal(plain.HCHA_D, ones.HCHA_D) and torch.equal(plain.HCHA_B, ones.HCHA_B)
    with pytest.raises(ValueError):
        generate_norm_HCHA(SimpleNamespace(x=torch.zeros(6, 1), edge_index=ei), False, torch.ones(4))


def _args(**kw):
    a = dict(All_num_layers=3, dropout=0.5, MLP_hidden=16, num_features=12, num_classes=4, HCHA_symdegnorm=False)
    a.update(kw)
    return SimpleNamespace(**a)


def test_model_without_the_new_attributes_is_todays():
    from allset_amd.baselines import HCHA
    torch.manual_seed(3)
    model = HCHA(_args())
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == [("convs.0.weight", (12, 16)), ("convs.0.bias", (16,)), ("convs.1.weight", (16, 16)), ("convs.1.bias", (16,)),
                   ("convs.2.weight", (16, 4)), ("convs.2.bias", (4,))]
    assert not any(c.use_attention for c in model.convs) and model.use_attention is False
    torch.manual_seed(3)
    off = HCHA(_args(HCHA_use_attention=False, heads=4, output_heads=2, HCHA_attn_drop=0.3))
    assert all(torch.equal(a, b) for a, b in zip(model.state_dict().values(), off.state_dict().values()))


def test_model_with_attention_follows_the_cegat_convention():
    from allset_amd.baselines import HCHA
    model = HCHA(_args(HCHA_use_attention=True, heads=4, output_heads=2, HCHA_attn_drop=0.3))
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == [("convs.0.weight", (12, 64)), ("convs.0.att", (1, 4, 32)), ("convs.0.bias", (64,)),
                   ("convs.1.weight", (64, 64)), ("convs.1.att", (1, 4, 32)), ("convs.1.bias", (64,)),
                   ("convs.2.weight", (64, 8)), ("convs.2.att", (1, 2, 8)), ("convs.2.bias", (4,))]
    assert [c.concat for c in model.convs] == [True, True, False] and all(c.dropout == 0.3 for c in model.convs)
    with pytest.raises(ValueError, match="symdegnorm"):
        HCHA(_args(HCHA_use_attention=True, HCHA_symdegnorm=True))


def test_driver_flags():
    from allset_amd.train import build_model, build_parser
    parse_args = build_parser().parse_args
    a = parse_args(["--method", "HCHA"])
    assert a.HCHA_use_attention is False and a.HCHA_attn_drop == 0.0
    a = parse_args(["--method", "HCHA", "--HCHA_use_attention", "--HCHA_attn_drop", "0.25", "--heads", "2"])
    assert a.HCHA_use_attention is True and a.HCHA_attn_drop == 0.25
    a.num_features, a.num_classes = 12, 4
    model = build_model(a, None)
    assert all(c.use_attention and c.dropout == 0.25 for c in model.convs) and model.convs[0].heads == 2


def test_abi_declares_the_entry_points():
    from allset_amd import _lib
    from allset_amd.build import SOURCES
    assert "hattn.hip" in SOURCES
    for sym, n_args in (("allset_hattn_supported", 0), ("allset_hattn_coef", 19), ("allset_hattn_hop", 22),
                        ("allset_hattn_bwd_vertex", 30), ("allset_hattn_bwd_edge", 7)):
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym]) == n_args, sym
