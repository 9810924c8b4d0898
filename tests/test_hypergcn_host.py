"""HyperGCN without a GPU: the driver's plumbing (``--method HyperGCN``, the two flags and their ``--no-`` forms, the preprocess
branch and its marker, ``build_model`` and its errors) and the width rule."""
import os
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hypergcn_cases as hc  # noqa: E402


def _block(pairs, n_v):
    v, e = pairs[0], pairs[1] + n_v
    ei = np.concatenate([np.stack([v, e]), np.stack([e, v])], axis=1)
    return torch.from_numpy(ei[:, np.lexsort((ei[1], ei[0]))])


def _data(name="hg_L2_fast_med"):
    from allset_amd.train import HypergraphData
    c = hc.spec(name)
    x, pairs, n_v, n_e = hc.raw_data(c)
    return c, pairs, HypergraphData(x=torch.from_numpy(x).float(), edge_index=_block(pairs, n_v), n_x=[n_v], num_hyperedges=[n_e])


def test_flags_are_live_and_default_to_the_reference():
    from allset_amd.train import BUILT_METHODS, build_parser
    assert "HyperGCN" in BUILT_METHODS and "MLP" not in BUILT_METHODS
    p = build_parser()
    a = p.parse_args(["--method", "HyperGCN"])
    assert a.HyperGCN_fast is True and a.HyperGCN_mediators is True          # reference train.py:284-285
    a = p.parse_args(["--method", "HyperGCN", "--HyperGCN_fast", "--HyperGCN_mediators"])
    assert a.HyperGCN_fast is True and a.HyperGCN_mediators is True
    a = p.parse_args(["--method", "HyperGCN", "--no-HyperGCN_fast"])
    assert a.HyperGCN_fast is False and a.HyperGCN_mediators is True
    a = p.parse_args(["--method", "HyperGCN", "--no-HyperGCN_mediators"])
    assert a.HyperGCN_fast is True and a.HyperGCN_mediators is False


@pytest.mark.parametrize("extra,fast,med", [([], True, True), (["--no-HyperGCN_fast"], False, True),
                                            (["--no-HyperGCN_fast", "--no-HyperGCN_mediators"], False, False)])
def test_preprocess_and_build_model(extra, fast, med):
    from allset_amd.baselines import HyperGCN
    from allset_amd.train import build_model, build_parser, preprocess
    c, pairs, data = _data()
    args = build_parser().parse_args(["--method", "HyperGCN", "--All_num_layers", "3", "--dname", "cora"] + extra)
    args.num_features, args.num_classes = c["F"], c["C"]
    data = preprocess(args, data)
    # ExtractV2E only: the vertex -> hyperedge half, no self-loop hyperedges; the marker holds the pairs with hyperedge ids from 0
    assert data.edge_index.shape[1] == pairs.shape[1] and int(data.edge_index[1].min()) == c["n_v"]
    want = pairs[:, np.lexsort((pairs[1], pairs[0]))]
    np.testing.assert_array_equal(data.HyperGCN_pairs.numpy(), want)
    model = build_model(args, data)
    assert isinstance(model, HyperGCN) and model.fast is fast and model.m is med and model.l == 3
    assert [(l.a, l.b) for l in model.layers] == [(12, 32), (32, 16), (16, 4)]
    assert all(l.reapproximate is (not fast) for l in model.layers)
    assert list(model.state_dict()) == [f"layers.{i}.{k}" for i in range(3) for k in ("W", "bias")]
    assert model.structure is None                                             # fast mode: built on the first forward
    args.dname = "citeseer"
    assert [(l.a, l.b) for l in build_model(args, data).layers] == [(12, 128), (128, 64), (64, 4)]


def test_width_rule():
    from allset_amd.baselines import hypergcn_widths
    assert hypergcn_widths(100, 1, 7, "cora") == [100, 7]
    assert hypergcn_widths(100, 2, 7, "cora") == [100, 16, 7]
    assert hypergcn_widths(100, 4, 7, None) == [100, 64, 32, 16, 7]
    assert hypergcn_widths(100, 6, 7, "pubmed") == [100, 256, 128, 64, 32, 16, 7]
    assert hypergcn_widths(100, 2, 6, "citeseer") == [100, 64, 6]
    assert hypergcn_widths(100, 4, 6, "citeseer") == [100, 256, 128, 64, 6]
    for L in range(1, 5):
        c = dict(L=L, F=9, C=3, dname="synthetic")
        assert hypergcn_widths(9, L, 3, "synthetic") == hc.widths(c)


def test_build_model_errors():
    from allset_amd.train import build_model, build_parser, preprocess
    c, pairs, data = _data()
    args = build_parser().parse_args(["--method", "HyperGCN"])
    args.num_features, args.num_classes = c["F"], c["C"]
    with pytest.raises(ValueError):
        build_model(args, None)
    with pytest.raises(ValueError, match="out of scope"):
        build_model(args, SimpleNamespace(edge_index=torch.from_numpy(pairs)))      # pairs that never saw preprocess, no x
    with pytest.raises(ValueError, match="preprocess"):
        build_model(args, data)                                                      # raw data: no marker
    args.method = "MLP"
    with pytest.raises(ValueError, match="MLP is out of scope"):
        build_model(args, data)
    # a singleton hyperedge under the default mediators: refused when the model is built, fine without mediators
    c, pairs, data = _data("hg_L2_fast_nomed")
    args = build_parser().parse_args(["--method", "HyperGCN"])
    args.num_features, args.num_classes = c["F"], c["C"]
    data = preprocess(args, data)
    with pytest.raises(ValueError, match="single member"):
        build_model(args, data)
    args.HyperGCN_mediators = False
    build_model(args, data)


def test_no_cpu_path():
    from allset_amd._lib import AllSetHipError
    from allset_amd.baselines import HyperGCN
    c, pairs, data = _data()
    model = HyperGCN(c["n_v"], torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], hc.args_of(c))
    with pytest.raises(AllSetHipError, match="no CPU path"):
        model(SimpleNamespace(x=data.x))
