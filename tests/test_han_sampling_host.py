"""CPU: mini-batch HAN without a device (allset_amd/han_sampling.py, csrc/han_sample.hip's entry points): the float64 restatement
against the recorded reference on every case, the fixtures against the live reference where it is present, the model's initial
parameters and ``state_dict`` layout, the header / binding / exported symbols of the new entry points, their argument checks (which
return before any launch), the host-side validation of the sampler's arguments, the parser's defaults against the reference's, and
``evaluate``'s last-batch-loss quirk with early stopping on a stub model."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import han_sampling_cases as sc  # noqa: E402
import han_sampling_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = dict(rtol=2e-5, atol=2e-5)
NEW_SYMBOLS = ["allset_han_sampling_supported", "allset_han_walk", "allset_han_block_rows", "allset_han_block_compact",
               "allset_han_block_hop_fwd", "allset_han_block_hop_bwd_stats", "allset_han_block_hop_bwd_src"]


def product_model(c):
    from allset_amd.han_sampling import HAN
    torch.manual_seed(c["seed"])
    return HAN(num_metapath=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=sc.DROPOUT)


def oracle_run(c, masks="case"):
    x, pairs, _, _ = sc.raw_data(c)
    blks = sc.blocks(c, pairs)
    sd64 = sc.perturb(product_model(c).state_dict(), c)
    if isinstance(masks, str):
        masks = sc.masks(c, blks)
        if masks is not None:
            masks = [tuple(torch.from_numpy(m) for m in pair) for pair in masks]
    sd = {k: v.clone().requires_grad_(True) for k, v in sd64.items()}
    hs = [torch.from_numpy(x)[b.src_ids].clone().requires_grad_(True) for b in blks]
    report = []
    out = orc.han_forward(sd, blks, hs, masks, report)
    (out * torch.from_numpy(sc.cotangent(c))).sum().backward()
    return out, hs, sd, min(report), blks


# ---- fixtures --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_initial_parameters_and_layout_equal_reference(name):
    from allset_amd import han
    c = sc.spec(name)
    fx = sc.load(sc.FILE)
    model = product_model(c)
    assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == [str(s) for s in fx[f"{name}/spec"]]
    assert sc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
    torch.manual_seed(c["seed"])
    full = han.HAN(num_meta_paths=2, in_size=c["F"], hidden_size=c["hidden"], out_size=c["C"], num_heads=c["heads"], dropout=sc.DROPOUT)
    assert [(k, tuple(v.shape)) for k, v in full.state_dict().items()] == [(k, tuple(v.shape)) for k, v in model.state_dict().items()]


@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_restatement_equals_reference(name):
    c = sc.spec(name)
    fx = sc.load(sc.FILE)
    out, hs, sd, margin, _ = oracle_run(c)
    print(f"{name}: kink margin {margin:.3e} (recorded {float(fx[name + '/margin']):.3e})")
    assert margin > sc.KINK_MARGIN and float(fx[f"{name}/margin"]) > sc.KINK_MARGIN
    sc.assert_result(out, fx, name, "out", **TOL)
    for i, h in enumerate(hs):
        sc.assert_result(h.grad, fx, name, f"grad_h{i}", **TOL)
    for k, v in sd.items():
        sc.assert_result(v.grad, fx, name, f"grad:{k}", **TOL)


def test_cases_cover_what_the_issue_lists():
    specs = {n: sc.spec(n) for n in sc.CASES}
    assert {c["heads"][0] for c in specs.values()} >= {1, 2, 8} and all(len(c["heads"]) == 1 for c in specs.values())
    assert any(c["train"] for c in specs.values()) and any(not c["train"] for c in specs.values())
    cora = specs["cora_hs"]
    assert (cora["n_v"], cora["n_e"], cora["F"], cora["B"], cora["k"], cora["bow"]) == (2708, 1579, 1433, 32, 20, True)
    c = specs["hs_h2"]
    _, pairs, n_v, n_e = sc.raw_data(c)
    seeds = sc.seed_nodes(c)
    assert len(set(seeds.tolist())) == c["B"]
    assert not np.isin(seeds[-2], pairs[0]) and seeds[-2] < n_v                 # an isolated vertex
    assert seeds[-1] >= n_v                                                      # a hyperedge node
    vev, eve = sc.blocks(c, pairs)
    for b in (vev, eve):
        assert b.n_dst == c["B"] and np.array_equal(b.src_ids[:b.n_dst].numpy(), seeds)
        deg = np.bincount(b.dst.numpy(), minlength=b.n_dst)
        assert deg.min() >= 1 and deg.max() <= c["k"] + 1
        loops = b.src == b.dst
        assert np.array_equal(np.bincount(b.dst[loops].numpy(), minlength=b.n_dst), np.ones(b.n_dst, dtype=np.int64))
    deg_v, deg_e = np.bincount(vev.dst.numpy()), np.bincount(eve.dst.numpy())
    assert deg_v[-1] == 1 and deg_v[-2] == 1 and deg_v[:-2].max() > 1           # the hyperedge node and the isolated vertex: loop alone
    assert (deg_e[:-1] == 1).all() and deg_e[-1] > 1 and eve.n_src > eve.n_dst   # EVE: vertices keep the loop alone
    assert vev.n_src > vev.n_dst


def test_explicit_dropout_factors_matter():
    c = sc.spec("hs_h2_train")
    assert float((oracle_run(c)[0] - oracle_run(c, masks=None)[0]).detach().abs().max()) > 1e-2


def test_fixtures_regenerate_byte_for_byte():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_han_sampling_fixtures as gen
    if not gen.available():
        pytest.skip("the reference's sources are not on this machine")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_han_sampling_fixtures.py"), "--check"], capture_output=True,
                         text=True)
    assert res.returncode == 0, res.stdout + res.stderr


def test_numpy_sampler_restatement_follows_the_exact_distribution():
    """The restatement the fixed blocks come from, against the closed form (a fixed numpy seed: deterministic)."""
    c = sc.spec("hs_h2")
    _, pairs, n_v, n_e = sc.raw_data(c)
    v2e, e2v = orc.adjacency(pairs, n_v, n_e)
    rng = np.random.default_rng(1)
    for mp, s in ((0, 0), (1, n_v + 2)):
        p = orc.endpoint_distribution(v2e, e2v, n_v, mp, s)
        N = 20000
        ends = np.array([orc.walk(v2e, e2v, n_v, mp, s, rng) for _ in range(N)])
        assert set(ends.tolist()) <= set(p)
        for u, pu in p.items():
            assert abs((ends == u).mean() - pu) <= 5 * np.sqrt(pu * (1 - pu) / N), (mp, s, u)
    assert orc.walk(v2e, e2v, n_v, 0, n_v + 2, rng) == -1 and orc.walk(v2e, e2v, n_v, 1, 0, rng) == -1
    assert orc.walk(v2e, e2v, n_v, 0, n_v - 1, rng) == -1                       # an isolated vertex


# ---- ABI -------------------------------------------------------------------------------------------------------------------------
def test_header_binding_and_exports_agree_for_the_new_entries():
    from allset_amd import _lib
    header = open(os.path.join(ROOT, "include", "allset_hip_ext.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
    for sym in NEW_SYMBOLS:
        m = re.search(r"\bint\s+" + sym + r"\s*\(([^;]*)\)\s*;", code)
        assert m, f"{sym} not declared"
        args = m.group(1).strip()
        n_args = 0 if args == "void" else args.count(",") + 1
        assert sym in _lib.SIGNATURES and len(_lib.SIGNATURES[sym]) == n_args, sym
        assert re.search(r" T " + sym + r"\b", out), f"{sym} not exported"
    assert _lib.load().allset_han_sampling_supported() == 1 and _lib.ABI_VERSION == 15


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call here fails its argument checks (status -1 or the unsupported status): nothing is launched, no device is needed."""
    from allset_amd import _lib
    lib = _lib.load()
    err = lambda: lib.allset_last_error().decode()
    assert lib.allset_han_walk(0, 0, 0, 0, 0, 4, 4, 0, 0, 3, 65, 1, 0, 0, 0) != 0 and "exceeds the built maximum" in err()
    assert lib.allset_han_walk(0, 0, 0, 0, 0, 4, 4, 0, 0, 3, 0, 1, 0, 0, 0) == -1 and "k >= 1" in err()
    assert lib.allset_han_walk(0, 0, 0, 0, 0, 4, 4, 0, 0, 3, 5, 1, 0, 0, 0) == -1 and "null" in err()
    assert lib.allset_han_walk(-1, 0, 0, 0, 0, 4, 4, 0, 0, 3, 5, 1, 0, 0, 0) == -1 and "metapath" in err()
    assert lib.allset_han_walk(0, 0, 0, 0, 0, 4, 4, 0, 0, 0, 5, 1, 0, 0, 0) == 0 and err() == ""           # B == 0: nothing to do
    assert lib.allset_han_block_rows(0, 0, 0, 3, 5, 0, 0, 0, 0) == -1 and "null" in err()
    assert lib.allset_han_block_rows(0, 0, 0, 3, 65, 0, 0, 0, 0) != 0 and "exceeds the built maximum" in err()
    assert lib.allset_han_block_compact(0, 0, 0, 0, 0, 0, 99, 3, 5, 4, 0, 0, 0) == -1 and "outside the slab" in err()
    assert lib.allset_han_block_compact(0, 0, 0, 0, 0, 0, 2, 3, 5, 4, 0, 0, 0) == -1 and "null" in err()
    z23 = [0] * 23
    a = list(z23); a[18], a[19], a[20], a[21] = 5, 4, 2, 4                      # n_dst > n_src
    assert lib.allset_han_block_hop_fwd(*a) == -1 and "first source rows" in err()
    a = list(z23); a[18], a[19], a[20], a[21] = 4, 5, 2, 512                    # H * C > 512
    rc = lib.allset_han_block_hop_fwd(*a)
    assert rc not in (0, -1) and "exceeds the built maximum" in err()
    a = list(z23); a[18], a[19], a[20], a[21] = 4, 5, 65, 1                     # H > 64
    assert lib.allset_han_block_hop_bwd_src(*a) not in (0, -1) and "exceeds the built maximum" in err()
    a = list(z23); a[18], a[19], a[20], a[21] = 4, 5, 2, 4                      # fine shapes, null pointers
    assert lib.allset_han_block_hop_fwd(*a) == -1 and "null" in err()
    assert lib.allset_han_block_hop_bwd_src(*a) == -1 and "null" in err()
    s = [0] * 18
    s[14], s[15], s[16] = 4, 2, 1024
    assert lib.allset_han_block_hop_bwd_stats(*s) not in (0, -1) and "exceeds the built maximum" in err()
    s[16] = 4
    assert lib.allset_han_block_hop_bwd_stats(*s) == -1 and "null" in err()
    # the full-graph entry points behind them (Python reaches them through the block ones only; C callers directly)
    z22 = [0] * 22
    for fn, i_p in ((lib.allset_han_hop_fwd, 9), (lib.allset_han_hop_bwd_src, 12)):
        a = list(z22); a[18], a[19], a[20] = 4, 2, 4                             # fine shapes, null pointers
        assert fn(*a) == -1 and "null" in err()
        a[20] = 512                                                              # H * C = 1024
        assert fn(*a) not in (0, -1) and "exceeds the built maximum" in err()
        a[20], a[i_p] = 4, 1.0                                                   # p_att = 1
        assert fn(*a) == -1 and "dropout p" in err()
    s[16] = 4
    assert lib.allset_han_hop_bwd_stats(*s) == -1 and "null" in err()
    s[16] = 512
    assert lib.allset_han_hop_bwd_stats(*s) not in (0, -1) and "exceeds the built maximum" in err()
    assert ctypes.sizeof(ctypes.c_void_p) == 8


# ---- host-side validation ----------------------------------------------------------------------------------------------------------
class _Walker:
    n_v, n_e, n, device = 5, 3, 8, torch.device("cpu")


def test_sampler_arguments_are_validated_on_the_host():
    from allset_amd import han_sampling as hs
    w = _Walker()
    assert hs.metapath_index(['Vs_E', 'E_Vs']) == 0 and hs.metapath_index(('Es_V', 'V_Es')) == 1 and hs.metapath_index('EVE') == 1
    with pytest.raises(ValueError, match="unknown metapath"):
        hs.metapath_index(['pa', 'ap'])
    with pytest.raises(ValueError, match="num_neighbors"):
        hs.HANSampler(w, hs.DEFAULT_METAPATHS, 65)
    with pytest.raises(ValueError, match="num_neighbors"):
        hs.HANSampler(w, hs.DEFAULT_METAPATHS, 0)
    s = hs.HANSampler(w, hs.DEFAULT_METAPATHS, 5, seed=3)
    assert s.metapaths == [0, 1]
    with pytest.raises(ValueError, match="duplicate seeds"):
        s.sample_blocks([1, 2, 1])
    with pytest.raises(ValueError, match="duplicate seeds"):
        s.sample_blocks(torch.tensor([4, 4]))
    with pytest.raises(ValueError, match="outside"):
        s.sample_blocks([1, 8])
    with pytest.raises(ValueError, match="outside"):
        s.sample_blocks(torch.tensor([-1, 2]))
    with pytest.raises(ValueError, match="integer"):
        s.sample_blocks([0.5, 1.0])
    with pytest.raises(ValueError, match="num_walks"):
        hs.random_walk_endpoints(w, 'VEV', [0], 65, 0, 0)
    assert s.counter == 0                                                        # a refused call takes no step counter


def test_model_rejects_what_is_not_built():
    from allset_amd import han, han_sampling as hs
    import torch.nn.functional as F
    with pytest.raises(ValueError):
        han.GATConv(4, 4, 2, activation=F.elu, allow_zero_in_degree=True)        # the full-batch conv is unchanged
    hs.GATConv(4, 4, 2, activation=F.elu, allow_zero_in_degree=True)
    with pytest.raises(ValueError, match="residual"):
        hs.GATConv(4, 4, 2, activation=F.elu, residual=True)
    with pytest.raises(ValueError, match="F.elu"):
        hs.GATConv(4, 4, 2, activation=None)
    model = hs.HAN(num_metapath=2, in_size=4, hidden_size=4, out_size=3, num_heads=[2, 2], dropout=0.0)
    with pytest.raises(ValueError, match="single-layer"):
        model([None, None], [torch.zeros(2, 4), torch.zeros(2, 4)])


def test_parser_defaults_equal_the_reference():
    from allset_amd import han_sampling as hs
    a = hs.build_parser().parse_args([]).__dict__
    want = dict(seed=1, batch_size=32, num_neighbors=20, lr=0.001, hidden_units=8, dropout=0.6, weight_decay=0.001, num_epochs=100,
                patience=10, runs=20, cuda=0, train_prop=0.5, valid_prop=0.25, feature_noise=1)
    assert {k: a[k] for k in want} == want
    assert a["dataset"] == "synthetic" and a["raw_data_dir"] is None and a["processed_data"] is None
    a = hs.setup(a)
    assert a["num_heads"] == [8] and a["device"] == "cuda:0"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import gen_han_sampling_fixtures as gen
    src = os.path.join(gen.HAN_DIR, "train_sampling.py")
    if gen.available():                                                          # (where the reference's sources are present)
        text = open(src).read()
        for k, v in want.items():
            m = re.search(r"add_argument\((?:'-s', )?'--" + k + r"'[^)]*default\s*=\s*([^,)\s]+)", text)
            assert m and float(m.group(1)) == float(v), k


# ---- evaluate ----------------------------------------------------------------------------------------------------------------------
def test_evaluate_returns_the_last_batch_loss_and_early_stopping_consumes_it(monkeypatch):
    from types import SimpleNamespace
    from allset_amd import han_sampling as hs
    made = []

    class StubSampler:
        def __init__(self, g, metapath_list, num_neighbors, seed=0):
            made.append((num_neighbors, seed))
            self.calls = []

        def sample_blocks(self, seeds, counter=None):
            self.calls.append((seeds.tolist(), counter))
            made.append(("call", seeds.tolist(), counter))
            return seeds, [SimpleNamespace(src_ids=seeds), SimpleNamespace(src_ids=seeds)]

    class StubModel(torch.nn.Module):
        def forward(self, blocks, hs_):
            return hs_[0]                                                        # the logits ARE the seeds' feature rows

    monkeypatch.setattr(hs, "HANSampler", StubSampler)
    # 5 nodes, 2 classes; batches of 2: [0, 1], [2, 3], [4].  Node 4 is confidently WRONG, the rest confidently right.
    features = torch.tensor([[9., 0.], [0., 9.], [9., 0.], [0., 9.], [0., 9.]])
    labels = torch.tensor([0, 1, 0, 1, 0])
    loss_fn = torch.nn.CrossEntropyLoss()
    model = StubModel()
    model.train()
    loss, acc, micro, macro = hs.evaluate(model, None, hs.DEFAULT_METAPATHS, 7, features, labels, torch.arange(5), loss_fn, 2, seed=5,
                                          counter=100)
    assert not model.training
    assert made[0] == (14, 5)                                                    # twice the training walks
    assert [m[1:] for m in made[1:]] == [([0, 1], 100), ([2, 3], 101), ([4], 102)]   # in order, no shuffling
    last = float(loss_fn(features[4:5], labels[4:5]))
    whole = float(loss_fn(features, labels))
    assert float(loss) == pytest.approx(last) and abs(last - whole) > 1.0        # the last batch's loss, not the mean
    assert acc == pytest.approx(4 / 5) and micro == pytest.approx(4 / 5)         # the scores are over ALL batches
    # early stopping consumes that loss: with the batch order reversed the same model is "better"
    loss2, acc2, _, _ = hs.evaluate(model, None, hs.DEFAULT_METAPATHS, 7, features, labels, torch.tensor([4, 0, 1, 2, 3]), loss_fn, 2)
    assert acc2 == pytest.approx(acc) and float(loss2) < float(loss)
    st = hs.EarlyStopping(patience=1)
    lin = torch.nn.Linear(1, 1)
    assert st.step(float(loss2), acc2, lin) is False
    assert st.step(float(loss), acc - 0.1, lin) is True                          # higher last-batch loss and lower accuracy: counts
    with pytest.raises(ValueError, match="no nodes"):
        hs.evaluate(model, None, hs.DEFAULT_METAPATHS, 7, features, labels, torch.arange(0), loss_fn, 2)
