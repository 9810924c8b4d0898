"""CPU: the host side of the HAN baseline (allset_amd/han.py): the metapath graphs' edge lists against a dense numpy restatement
(doubled self-loops included), the zero-in-degree error, the driver's parser defaults and settings, its split, the reference's
early-stopping rule on a scripted series, accuracy / micro / macro F1 against a hand count, and train.py's method list unchanged."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_cases as hc  # noqa: E402


@pytest.mark.parametrize("name", ["han_h2_L1", "han_h8_h1_L2", "cora_han"])
def test_metapath_edges_equal_dense_restatement(name):
    from allset_amd.han import metapath_edges
    c = hc.spec(name)
    _, pairs, n_v, n_e = hc.raw_data(c)
    got = metapath_edges(torch.from_numpy(pairs), n_v, n_e)
    want = hc.dense_metapath_edges(pairs, n_v, n_e)
    assert len(got) == 2
    for (r, cc), (wr, wc) in zip(got, want):
        assert r.dtype == torch.int64 and np.array_equal(r.numpy(), wr) and np.array_equal(cc.numpy(), wc)
    n = n_v + n_e
    (r, cc), (r2, c2) = got
    loops = np.bincount(r[r == cc].numpy(), minlength=n)
    members = np.unique(pairs[0])
    assert (loops[members] == 2).all()                                     # H H^T has the diagonal already: appended, not replaced
    assert (loops[np.setdiff1d(np.arange(n), members)] == 1).all()         # isolated vertices and every hyperedge node: the loop alone
    assert int(r.max()) == n - 1 and int(r[:-n].max()) < n_v and int(r2[:-n].min()) >= n_v
    assert np.array_equal(r[-n:].numpy(), np.arange(n)) and np.array_equal(cc[-n:].numpy(), np.arange(n))


def test_zero_in_degree_raises_like_dgl():
    from allset_amd.han import MetapathGraph
    src, dst = torch.tensor([0, 1, 2]), torch.tensor([1, 0, 1])
    with pytest.raises(ValueError, match="0-in-degree"):
        MetapathGraph(src, dst, 3)


def test_node_features_pad_hyperedges_with_zero_rows_and_unlabelled():
    from types import SimpleNamespace
    from allset_amd.han import node_features
    data = SimpleNamespace(x=torch.ones(3, 2), y=torch.tensor([0, 1, 0]), n_x=[3], num_hyperedges=[2])
    x, y = node_features(data)
    assert x.shape == (5, 2) and float(x[3:].abs().sum()) == 0.0 and y.tolist() == [0, 1, 0, -1, -1]


def test_parser_defaults_and_settings():
    from allset_amd import han
    a = han.build_parser().parse_args([]).__dict__
    assert (a["seed"], a["runs"], a["cuda"], a["feature_noise"], a["train_prop"], a["valid_prop"]) == (1, 20, 0, 1, 0.5, 0.25)
    assert a["dataset"] == "synthetic"
    a = han.setup(a)
    assert (a["lr"], a["num_heads"], a["hidden_units"], a["dropout"], a["weight_decay"], a["num_epochs"], a["patience"]) == \
        (0.005, [8], 8, 0.6, 0.001, 200, 100)
    assert han.setup(han.build_parser().parse_args(["--num_epochs", "30"]).__dict__)["num_epochs"] == 30


def test_split_is_over_labelled_nodes_and_follows_numpy_seed():
    from allset_amd.han import rand_train_test_idx
    label = torch.tensor([0, 1, -1, 2, 0, 1, -1, 2, 0, 1, 2, 0])
    np.random.seed(3)
    s = rand_train_test_idx(label, 0.5, 0.25)
    np.random.seed(3)
    perm = np.random.permutation(10)
    labelled = np.flatnonzero(label.numpy() != -1)
    assert s["train"].tolist() == labelled[perm[:5]].tolist()
    assert s["valid"].tolist() == labelled[perm[5:7]].tolist()
    assert s["test"].tolist() == labelled[perm[7:]].tolist()
    np.random.seed(4)
    assert rand_train_test_idx(label, 0.5, 0.25)["train"].tolist() != s["train"].tolist()


def test_early_stopping_follows_the_reference_rule():
    from allset_amd.han import EarlyStopping
    model = torch.nn.Linear(1, 1)
    st = EarlyStopping(patience=2)
    seen = []
    #          loss  acc   -> (counter, saves, best_loss, best_acc, stop)
    script = [(1.0, 0.5, (0, 1, 1.0, 0.5, False)),      # first step: saved
              (0.9, 0.4, (0, 1, 0.9, 0.5, False)),      # better loss, worse acc: bests updated separately, NOT saved
              (0.95, 0.45, (1, 1, 0.9, 0.5, False)),    # worse in both: counts
              (0.9, 0.5, (0, 2, 0.9, 0.5, False)),      # ties in both: saved, count reset
              (1.2, 0.6, (0, 2, 0.9, 0.6, False)),      # worse loss, better acc: reset, not saved
              (1.0, 0.55, (1, 2, 0.9, 0.6, False)),
              (1.0, 0.55, (2, 2, 0.9, 0.6, True))]      # patience reached
    for i, (loss, acc, want) in enumerate(script):
        with torch.no_grad():
            model.weight.fill_(float(i))
        stop = st.step(loss, acc, model)
        seen.append((st.counter, st.saves, st.best_loss, st.best_acc, stop))
        assert seen[-1] == want, (i, seen[-1], want)
    st.load_checkpoint(model)
    assert float(model.weight) == 3.0                   # the state of the last save, kept in memory


def test_scores_against_a_hand_count():
    from allset_amd.han import score
    labels = torch.tensor([0, 0, 0, 1, 1, 2, 2, 2])
    pred = torch.tensor([0, 0, 1, 1, 2, 2, 2, 0])
    logits = torch.nn.functional.one_hot(pred, 3).float()
    acc, micro, macro = score(logits, labels)
    # class 0: tp 2 fp 1 fn 1 -> 2/3; class 1: tp 1 fp 1 fn 1 -> 1/2; class 2: tp 2 fp 1 fn 1 -> 2/3
    assert acc == pytest.approx(5 / 8) and micro == pytest.approx(5 / 8) and macro == pytest.approx((2 / 3 + 1 / 2 + 2 / 3) / 3)
    # a class that is predicted but absent from the labels counts in the macro mean with F1 = 0
    acc, micro, macro = score(torch.nn.functional.one_hot(torch.tensor([0, 2]), 3).float(), torch.tensor([0, 0]))
    assert acc == 0.5 and macro == pytest.approx((2 / 3 + 0.0) / 2)


def test_train_py_method_list_is_unchanged():
    from allset_amd import train
    assert train.BUILT_METHODS == ('AllSetTransformer', 'AllDeepSets', 'HGNN', 'HCHA', 'HNHN', 'CEGCN', 'CEGAT', 'UniGCNII', 'HyperGCN',
                                   'UniGCN', 'UniGCN2', 'UniGIN', 'UniSAGE', 'UniGAT')
    assert 'HAN' not in train.BUILT_METHODS
