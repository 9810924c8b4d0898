"""HyperGCN on the CPU: the float64 restatement (tests/hypergcn_oracle.py) against the reference's recorded results
(tests/golden/baselines_hypergcn*.npz) at the project's 2e-5 -- every adjacency, logits, d/dx and every parameter gradient, in eval
mode and in training mode with explicit dropout factors; its dictionary-free sparse form against its dense form; the product's
initial parameters and layout against the recorded checksum; the refused inputs; and the two a-priori criteria every case must meet
(relu-kink margin, projection-gap margin), computed by the restatement alone."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hypergcn_cases as hc  # noqa: E402
import hypergcn_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILE_OF = {name: file for file, names in hc.FILES.items() for name in names}


def oracle_run(c, fx, name):
    """The restatement on the case with the recorded projection vectors and the case's parameters (the product's initial draw --
    the recorded checksum ties it to the reference's -- plus the seeded perturbation, rounded to fp32 as the reference held them)."""
    from allset_amd.baselines import HyperGCN
    x, pairs, n_v, n_e = hc.raw_data(c)
    members = hc.member_lists(pairs, n_e)
    torch.manual_seed(c["seed"])
    init = HyperGCN(n_v, torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], hc.args_of(c)).state_dict()
    assert hc.checksum(init) == str(fx[f"{name}/chk"])
    sd = {k: v.float().double().requires_grad_(True) for k, v in hc.perturb(init, c).items()}
    xo = torch.from_numpy(x).float().double().requires_grad_(True)
    rvs = [fx[f"{name}/rv{i}"] for i in range(len(hc.rv_sizes(c)))]
    masks = [torch.from_numpy(m) for m in hc.masks(c)]
    margins, gaps, structures = [], [], []
    logits = orc.forward(sd, xo, members, n_v, c["L"], c["fast"], c["med"], rvs, masks, c["train"], margins, gaps, structures)
    G = torch.from_numpy(hc.cotangent(c, n_v))
    (logits * G).sum().backward()
    return dict(logits=logits.detach(), x=xo, sd=sd, margins=margins, gaps=gaps, structures=structures, members=members, n_v=n_v)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_restatement_matches_recorded_reference(name):
    c = hc.spec(name)
    fx = hc.load(FILE_OF[name])
    r = oracle_run(c, fx, name)

    def scale(k):
        kind, v = hc.result(fx, name, k)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    hc.assert_result(r["logits"], fx, name, "logits", rtol=2e-5, atol=2e-5 * scale("logits"))
    hc.assert_result(r["x"].grad, fx, name, "grad_x", rtol=2e-5, atol=2e-5 * scale("grad_x"))
    for k, p in r["sd"].items():
        hc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=2e-5, atol=2e-5 * scale(f"grad:{k}"))
    for i, (S, I, _) in enumerate(r["structures"]):
        A, _ = orc.dense_A(r["n_v"], r["members"], S, I, c["med"])
        if f"{name}/A{i}:indices" in fx:
            idx, val = fx[f"{name}/A{i}:indices"].astype(np.int64), fx[f"{name}/A{i}:values"]
            assert idx.shape[1] == np.count_nonzero(A)
            np.testing.assert_allclose(A[idx[0], idx[1]], val, rtol=2e-5, atol=2e-5)
        else:
            assert int(fx[f"{name}/A{i}:nnz"]) == np.count_nonzero(A)
            pr = np.random.default_rng(r["n_v"]).standard_normal((r["n_v"], 3))
            np.testing.assert_allclose(A @ pr, fx[f"{name}/A{i}:matvec"], rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("name", list(hc.CASES))
def test_sparse_form_equals_dense_form(name):
    c = hc.spec(name)
    r = oracle_run(c, hc.load(FILE_OF[name]), name)
    h = np.random.default_rng(1).standard_normal((r["n_v"], 5))
    for S, I, dinv in r["structures"]:
        A, _ = orc.dense_A(r["n_v"], r["members"], S, I, c["med"])
        trip = orc.triplets(r["members"], S, I, c["med"])
        np.testing.assert_allclose(orc.sparse_dinv(r["n_v"], trip), dinv, rtol=1e-13)
        np.testing.assert_allclose(orc.sparse_apply(r["n_v"], trip, h), A @ h, rtol=1e-12, atol=1e-13)
        np.testing.assert_allclose(A, A.T, rtol=0, atol=1e-15)                 # symmetric: the hop is its own backward


@pytest.mark.parametrize("name", list(hc.CASES))
def test_cases_keep_the_a_priori_margins(name):
    """Both criteria for every case, from the restatement alone.  Exact ties (gap 0) are admitted in the fast tie cases only."""
    c = hc.spec(name)
    r = oracle_run(c, hc.load(FILE_OF[name]), name)
    print(name, "relu margins", ["%.3e" % m for m in r["margins"]])
    assert min(r["margins"]) > hc.RELU_MARGIN
    rel = []
    for layer in r["gaps"]:
        for t in layer:
            if t is None:
                continue
            for gap in t[:2]:
                if gap == 0.0:
                    assert c["ties"] and c["fast"], (name, "an exact tie outside the fast tie cases")
                    continue
                rel.append(gap / t[2])
    print(name, "smallest relative projection gap %.3e" % min(rel), "margin %.3e" % hc.GAP_MARGIN)
    assert min(rel) > hc.GAP_MARGIN
    if c["ties"]:
        S, I, _ = r["structures"][0]
        first = [v for v in r["members"][3] if v in (0, 1)][0]
        assert int(I[3]) == first                                           # the joint arg-min goes to the earlier pair of the list
        assert int(S[4]) == int(I[4]) == r["members"][4][0] and len(r["members"][4]) == 3      # S = I, k = 3
    if c["bow"]:
        x, _, _, _ = hc.raw_data(c)
        assert int((x != 0).sum(1).max()) <= hc.GAP_TERMS
    if not c["fast"]:
        assert max(a + b for a, b in zip(hc.widths(c)[:-1], hc.widths(c)[1:])) <= hc.GAP_TERMS


def test_case_coverage():
    specs = {n: hc.spec(n) for n in hc.CASES}
    assert {c["L"] for c in specs.values()} >= {1, 2, 3}
    assert {(c["fast"], c["med"]) for c in specs.values()} == {(True, True), (True, False), (False, True), (False, False)}
    assert any(c["train"] and c["fast"] for c in specs.values()) and any(c["train"] and not c["fast"] for c in specs.values())
    assert all(not c["med"] for c in specs.values() if c["singletons"]) and all(c["fast"] for c in specs.values() if c["ties"])
    c = specs["hg_L2_fast_nomed"]
    _, pairs, n_v, n_e = hc.raw_data(c)
    sizes = np.bincount(pairs[1], minlength=n_e)
    assert sizes[0] == 2 and sizes[1] == 3 and (sizes == 1).sum() == 2 and sizes.max() <= 8
    mem = hc.member_lists(pairs, n_e)
    assert sorted(mem[5]) == sorted(mem[6]) == sorted(mem[7])
    assert set(range(n_v)) - set(pairs[0].tolist()) >= {7, 30, n_v - 1}
    assert hc.widths(specs["hg_L3_citeseer"]) == [12, 128, 64, 4] and hc.widths(specs["hg_L3_slow_med_train"]) == [12, 32, 16, 4]


def test_state_dict_layout_matches_reference():
    from allset_amd.baselines import HyperGCN, HyperGraphConvolution
    for name in ("hg_L1_fast_med", "hg_L3_citeseer", "hg_L3_slow_med_train"):
        c = hc.spec(name)
        fx = hc.load(FILE_OF[name])
        _, pairs, n_v, _ = hc.raw_data(c)
        torch.manual_seed(c["seed"])
        model = HyperGCN(n_v, torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], hc.args_of(c))
        assert [f"{k}|{list(v.shape)}|{v.dtype}" for k, v in model.state_dict().items()] == list(fx[f"{name}/spec"])
        assert hc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
        torch.manual_seed(c["seed"])
        model.reset_parameters()
        assert hc.checksum(model.state_dict()) == str(fx[f"{name}/chk"])
        assert all(layer.reapproximate == (not c["fast"]) for layer in model.layers)
    conv = HyperGraphConvolution(24, 32)
    assert float(conv.W.abs().max()) <= 32 ** -0.5 and float(conv.bias.abs().max()) <= 32 ** -0.5
    assert repr(conv) == "HyperGraphConvolution (24 -> 32)"


def test_refused_inputs_raise():
    from allset_amd.baselines import HyperGCN
    c = hc.spec("hg_L2_fast_nomed")
    _, pairs, n_v, _ = hc.raw_data(c)
    args = hc.args_of(c)
    HyperGCN(n_v, torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], args)            # singletons are fine without mediators
    args.HyperGCN_mediators = True
    first = int(np.flatnonzero(np.bincount(pairs[1]) == 1)[0])
    with pytest.raises(ValueError, match=f"hyperedge {first} has a single member"):
        HyperGCN(n_v, torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], args)
    c = hc.spec("hg_L2_fast_med")
    _, pairs, n_v, _ = hc.raw_data(c)
    dup = np.concatenate([pairs, pairs[:, 5:6]], axis=1)
    for med in (True, False):
        args = hc.args_of(c)
        args.HyperGCN_mediators = med
        with pytest.raises(ValueError, match=f"vertex {pairs[0, 5]} occurs 2 times in hyperedge {pairs[1, 5]}"):
            HyperGCN(n_v, torch.from_numpy(dup), None, c["F"], c["L"], c["C"], args)
    with pytest.raises(ValueError):
        HyperGCN(n_v, {0: [1, 2]}, None, c["F"], c["L"], c["C"], hc.args_of(c))           # the reference's dict is not taken
    with pytest.raises(ValueError):
        HyperGCN(5, torch.from_numpy(pairs), None, c["F"], c["L"], c["C"], hc.args_of(c))  # vertex ids beyond V


def test_fixtures_regenerate_byte_for_byte():
    sys.path.insert(0, ROOT)
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip("the reference tree is not on this machine")
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_hypergcn_fixtures.py"), "--check"], cwd=ROOT,
                         capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert res.stdout.count("matches") == len(hc.FILES)
