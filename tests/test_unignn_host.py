"""CPU: the host side of the UniGNN baselines (``--method UniGCN | UniGCN2 | UniGIN | UniSAGE | UniGAT``): the driver's flags and the
names the convs read from ``args``, ``build_model`` on preprocessed data and its errors on anything else, the refusals, the one-group
optimizer, and the no-CPU-path error of a forward."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

METHODS = ("UniGCN", "UniGCN2", "UniGIN", "UniSAGE", "UniGAT")


def _data(n_v=30, n_e=10, F=6, C=3, seed=0):
    from allset_amd.train import HypergraphData
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(0, n_v - 2, (40,), generator=g)
    e = torch.randint(0, n_e, (40,), generator=g) + n_v
    e[0], v[1] = n_v + n_e - 1, n_v - 3
    ei = torch.cat([torch.stack([v, e]), torch.stack([e, v])], dim=1)
    return HypergraphData(x=torch.randn(n_v, F, generator=g), edge_index=ei, y=torch.arange(n_v) % C, n_x=[n_v], num_hyperedges=[n_e])


def _args(method, extra=()):
    from allset_amd.train import build_parser
    args = build_parser().parse_args(["--method", method, *extra])
    args.num_features, args.num_classes = 6, 3
    return args


def test_methods_and_flags():
    from allset_amd.train import BUILT_METHODS, UNIGNN_CONV_METHODS, UNIGNN_METHODS, build_parser
    assert UNIGNN_CONV_METHODS == METHODS and UNIGNN_METHODS == ("UniGCNII",)
    assert set(METHODS) <= set(BUILT_METHODS) and "MLP" not in BUILT_METHODS
    a = build_parser().parse_args([])
    assert (a.UniGNN_first_aggregate, a.UniGNN_second_aggregate, a.UniGNN_activation) == ("mean", "sum", "relu")
    assert (a.UniGNN_input_drop, a.UniGNN_attn_drop, a.UniGNN_use_norm) == (0.6, 0.0, False)
    a = build_parser().parse_args(["--UniGNN_first_aggregate", "sum", "--UniGNN_second_aggregate", "mean", "--UniGNN_activation", "prelu",
                                   "--UniGNN_input_drop", "0.1", "--UniGNN_attn_drop", "0.3", "--UniGNN_use-norm"])
    assert (a.UniGNN_first_aggregate, a.UniGNN_second_aggregate, a.UniGNN_activation) == ("sum", "mean", "prelu")
    assert (a.UniGNN_input_drop, a.UniGNN_attn_drop, a.UniGNN_use_norm) == (0.1, 0.3, True)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--UniGNN_activation", "gelu"])


@pytest.mark.parametrize("method", METHODS)
def test_build_model_on_preprocessed_data(method):
    from allset_amd import baselines
    from allset_amd.optim import FusedAdam
    from allset_amd.train import build_model, make_optimizer, preprocess
    args = _args(method, ["--heads", "2", "--MLP_hidden", "8", "--All_num_layers", "3", "--UniGNN_use-norm", "--dropout", "0.3"])
    data = preprocess(args, _data())
    model = build_model(args, data)
    assert isinstance(model, baselines.UniGNN) and type(model.conv_out) is baselines.UNIGNN_CONVS[method]
    assert args.model_name == method and args.use_norm is True and args.first_aggregate == "mean" and args.activation == "relu"
    assert args.degV is args.UniGNN_degV and args.degE is args.UniGNN_degE and args.degV.shape == (30, 1)
    assert len(model.convs) == 2 and model.convs[0].heads == 2 and model.conv_out.heads == 1
    assert model.convs[1].W.in_features == 16 and model.conv_out.W.out_features == 3
    assert (model.input_drop.p, model.dropout.p) == (0.6, 0.3)
    assert next(iter(model.state_dict())).startswith("conv_out.")
    assert repr(model.convs[0]) == f"{type(model.conv_out).__name__}(6, 8, heads=2)"
    opt = make_optimizer(args, model)
    assert isinstance(opt, FusedAdam) and len(opt.param_groups) == 1
    assert opt.param_groups[0]["lr"] == args.lr and opt.param_groups[0]["weight_decay"] == args.wd
    before = [p.clone() for p in model.parameters()]
    model.reset_parameters()
    assert any(not torch.equal(a, b) for a, b in zip(before, model.parameters()))
    if method == "UniGIN":
        assert float(model.conv_out.eps) == 0.0
    if method == "UniGAT":
        assert model.conv_out.att_v.shape == (1, 1, 3) and model.convs[0].att_e.shape == (1, 2, 8)
    with pytest.raises(baselines.AllSetHipError, match="no CPU path"):
        model(data.x)
    with pytest.raises(baselines.AllSetHipError, match="no CPU path"):
        model(data)                                                                # a data object with .x


@pytest.mark.parametrize("method", METHODS)
def test_build_model_insists_on_preprocess(method):
    from allset_amd.train import build_model, preprocess
    args = _args(method)
    with pytest.raises(ValueError, match="preprocess"):
        build_model(args, _data())
    with pytest.raises(ValueError, match="preprocess"):
        build_model(args, None)
    other = preprocess(_args("HCHA"), _data())                                     # another branch's data
    with pytest.raises(ValueError, match="preprocess"):
        build_model(args, other)


def test_refusals_through_the_driver():
    from allset_amd.train import build_model, preprocess
    for extra, what in ((["--UniGNN_first_aggregate", "max"], "first_aggregate"), (["--UniGNN_attn_drop", "0.2"], "attention coefficients")):
        args = _args("UniGAT", extra)
        with pytest.raises(NotImplementedError, match=what):
            build_model(args, preprocess(args, _data()))
    args = _args("UniSAGE", ["--UniGNN_second_aggregate", "max"])
    with pytest.raises(NotImplementedError, match="second_aggregate"):
        build_model(args, preprocess(args, _data()))
    args = _args("UniGCN", ["--UniGNN_attn_drop", "0.2"])                          # unused outside UniGAT, as in the reference
    build_model(args, preprocess(args, _data()))


def test_mlp_keeps_its_message_and_missing_scales_are_named():
    from types import SimpleNamespace
    from allset_amd.baselines import UniGCNConv, UniGNN
    from allset_amd.train import build_model, run
    with pytest.raises(ValueError, match="MLP is out of scope"):
        build_model(_args("MLP"), _data())
    with pytest.raises(ValueError, match="out of scope"):
        run(_args("MLP"))
    args = SimpleNamespace(model_name="UniGXX", attn_drop=0.0)
    with pytest.raises(ValueError, match="model_name"):
        UniGNN(args, 4, 4, 3, 2, 1, None, None)
    conv = UniGCNConv(SimpleNamespace(first_aggregate="mean"), 4, 4, heads=1)
    with pytest.raises(Exception, match="no CPU path|degV"):
        conv(torch.zeros(3, 4), torch.zeros(2, dtype=torch.long), torch.zeros(2, dtype=torch.long))


def test_run_needs_a_gpu(monkeypatch):
    from allset_amd.train import run
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    args = _args("UniGIN", ["--epochs", "1", "--runs", "1"])
    with pytest.raises(RuntimeError, match="no CPU path"):
        run(args)
