"""CPU: every case tests/test_gpu_hop_structures.py runs, vouched for from the float64 restatements alone -- finite reference outputs
and gradients, a leaky-relu logit margin of at least 1/16, a relu pre-activation margin of at least 0.25 -- and the structures'
own properties (row-length multisets, empty runs, n % 7, duplicates).  The case lists are imported from tests/hop_structures.py, the
module the GPU file imports them from."""
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_structures as hs  # noqa: E402


def _deg(ei, n, row):
    return np.bincount(ei[row], minlength=n)


# ---- the structures are what their names say ---------------------------------------------------------------------------------------
def test_structures_have_the_properties_they_are_named_for():
    S = hs.structures()
    assert list(S) == ["empty", "single", "tiny", "rows5", "one_row", "one_col", "dups", "edge_empties", "wide", "tall", "lengths",
                       "flat50"]
    for name, (n_src, n_dst, ei) in S.items():
        assert ei.dtype == np.int64 and ei.shape[0] == 2 and max(n_src, n_dst) <= 700 and ei.shape[1] <= 6000, name
        if ei.shape[1]:
            assert 0 <= ei[0].min() and ei[0].max() < n_src and 0 <= ei[1].min() and ei[1].max() < n_dst, name
    assert S["empty"][:2] == (5, 3) and S["empty"][2].shape == (2, 0)
    assert S["single"][:2] == (1, 1) and S["single"][2].tolist() == [[0], [0]]
    assert S["tiny"][:2] == (3, 2) and S["tiny"][2].shape[1] == 4
    assert S["rows5"][:2] == (6, 5) and S["rows5"][2].shape[1] == 20 and _deg(S["rows5"][2], 5, 1).tolist() == [4] * 5   # 4 waves + 1
    n_src, n_dst, ei = S["one_row"]
    assert (n_src, n_dst, ei.shape[1]) == (300, 37, 1500) and len(set(ei[1].tolist())) == 1
    assert Counter(_deg(ei, 37, 1).tolist()) == Counter({0: 36, 1500: 1})
    n_src, n_dst, eit = S["one_col"]
    assert (n_src, n_dst) == (37, 300) and np.array_equal(eit, ei[::-1]) and len(set(eit[0].tolist())) == 1
    n_src, n_dst, ei = S["dups"]
    pairs = Counter(zip(ei[0].tolist(), ei[1].tolist()))
    assert len(pairs) == 50 and set(pairs.values()) == {8}
    n_src, n_dst, ei = S["edge_empties"]
    deg = _deg(ei, n_dst, 1)
    assert (n_src, n_dst) == (90, 100) and not deg[:3].any() and not deg[60:].any() and deg[3:60].all()
    deg_s = _deg(ei, n_src, 0)
    assert not deg_s[:5].any() and not deg_s[80:].any() and deg_s[5:80].any()          # and of the transposed CSR of the backward
    assert S["wide"][:2] == (700, 9) and S["tall"][:2] == (9, 700)
    assert (_deg(S["tall"][2], 700, 1) == 0).any() and _deg(S["wide"][2], 9, 1).min() >= 200
    n_src, n_dst, ei = S["flat50"]
    deg = _deg(ei, n_dst, 1)
    assert n_dst == 50 and n_dst % 7 != 0 and ei.shape[1] / n_dst < 6 and deg[:8].tolist() == [0, 0, 1, 9, 0, 0, 0, 17]
    assert deg.max() > 8                                                   # a row longer than the narrowest lane group


@pytest.mark.parametrize("T", [hs.CSR_LONG_T, hs.LOO_LONG_T])
def test_lengths_rows_sit_on_the_chunk_and_threshold_boundaries(T):
    n_src, n_dst, ei = hs.structures(T)["lengths"]
    deg = _deg(ei, n_dst, 1).tolist()
    assert deg == [0, 0, 1, 9, 0, 0, 0, 17, 2, 63, 64, 65, 0, 127, 128, 129, 1, 0, T - 1, T, T + 1, 0, 0]
    for t in range(n_dst):                                                 # distinct sources within a row
        assert len(set(ei[0][ei[1] == t].tolist())) == deg[t]


def test_thresholds_are_the_codes_own():
    """``LOO_LONG_T`` is the library's; ``CSR_LONG_T`` is the ``max_deg > 256`` of ``ops.long_rows_first_order``, the only
    row-length rule on the CSR hops' path: a CSR whose longest row has 256 incidences keeps the natural order, 257 reorders."""
    from allset_amd import ops
    assert ops.loo_long_threshold() == hs.LOO_LONG_T
    for longest, reordered in ((hs.CSR_LONG_T, False), (hs.CSR_LONG_T + 1, True)):
        deg = torch.tensor([longest] + [2] * 99)
        rowptr = torch.zeros(101, dtype=torch.int32)
        rowptr[1:] = torch.cumsum(deg, 0)
        order = ops.long_rows_first_order(rowptr, 100, int(deg.sum()), longest)
        assert (order is not None) == reordered


def test_width_classes_straddle_every_lane_group_boundary():
    vec, scalar = hs.width_classes(True), hs.width_classes(False)
    assert vec == [4, 12, 32, 36, 64, 68, 128, 132, 256, 260, 512] and scalar == [1, 3, 7, 9, 18, 33, 70, 257]
    assert all(d % 4 == 0 for d in vec) and all(d % 4 for d in scalar)
    assert {hs.pick_lpr(d, 4) for d in vec} == {8, 16, 32, 64} and {hs.pick_lpr(d, 1) for d in scalar} == {8, 16, 32, 64}
    for lo, hi in ((32, 36), (64, 68), (128, 132), (256, 260)):            # both sides of a boundary (the last: the column-chunk loop)
        assert lo in vec and hi in vec
    assert hs.width_classes(True, built=lambda d: d <= 256) == vec[:9]


def _sweep_rule(cases, vec_of):
    """every structure at two widths, one per vector path; every width class at edge_empties and at lengths."""
    by = {}
    for c in cases:
        by.setdefault(c.struct, set()).add(vec_of(c))
    for name in hs.structures():
        assert {True, False} <= {v for v, _ in by[name]}, name
    for name in ("edge_empties", "lengths"):
        assert {d for _, d in by[name]} >= set(hs.VEC_WIDTHS) | set(hs.SCALAR_WIDTHS), name


def _dropout_rule(cases, width):
    for p in (0.5, 0.3):                                                   # the 8-bit and the 16-bit mask form
        assert any(c.p == p and width(c) % 2 == 1 for c in cases) and any(c.p == p and width(c) % 4 == 0 for c in cases)


# ---- family 1 -----------------------------------------------------------------------------------------------------------------------
def test_hconv_case_list_covers_the_dispatcher():
    scaled = [c for c in hs.HCONV_CASES if not c.weighted]
    weighted = [c for c in hs.HCONV_CASES if c.weighted]
    for cases in (scaled, weighted):
        _sweep_rule(cases, lambda c: (c.d % 4 == 0, c.d))
        _dropout_rule(cases, lambda c: c.d)
        assert {c.variant for c in cases} == {None, 1, 2} and {c.act for c in cases} == {None, "relu", "elu"}
    assert {(c.direction, c.has_r, c.has_s) for c in scaled} == {(a, b, d) for a in ("v2e", "e2v") for b in (True, False) for d in (True, False)}
    assert {c.has_r for c in weighted} == {True, False}
    # the short-row kernel: every lane-group width with every scale form (forward: r given or not; the weighted form: w), over the
    # adversarial row structures
    flat = {(hs.pick_lpr(c.d, 4), "w" if (c.weighted and c.has_r) else "r" if (not c.weighted and c.has_r) else "none", c.struct)
            for c in hs.HCONV_CASES if c.variant == 2}
    for lpr in (8, 16, 32, 64):
        for sc in ("none", "r", "w"):
            assert any(f[0] == lpr and f[1] == sc for f in flat), (lpr, sc)
            assert any(f == (lpr, sc, name) for f in flat for name in ("flat50", "lengths")), (lpr, sc)
    assert all(hs.hconv_flat_ok(c.d) for c in hs.HCONV_CASES if c.variant == 2)
    assert all(not hs.hconv_flat_ok(d) for _, d in hs.HCONV_VARIANT_ERRORS)
    assert any(c.d > 256 and c.d % 4 == 0 for c in scaled)                 # the column-chunk loop with VEC = 4
    rows = {(hs.pick_lpr(c.d, 4), c.has_r) for c in weighted if c.variant == 1 and c.d % 4 == 0}
    assert rows >= {(l, True) for l in (8, 16, 32, 64)}                    # one wavefront per row with the weight stream, every width


@pytest.mark.parametrize("c", hs.HCONV_CASES, ids=lambda c: c.id)
def test_hconv_reference_is_finite_and_clear_of_the_kinks(c):
    inp = hs.hconv_inputs(c)
    y, grads, margin = hs.hconv_reference(c, inp, hs.host_mask((inp["n_t"], c.d), c.p, 1))
    assert y.shape == (inp["n_t"], c.d) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert margin >= hs.RELU_MARGIN
    if c.act == "relu":
        assert bool((y > 0).any()) or c.d == 1
        assert bool((y == 0).any()) or c.d == 1                            # both branches (odd columns are clipped)


# ---- family 2 -----------------------------------------------------------------------------------------------------------------------
def test_gat_case_list_covers_the_dispatcher():
    _sweep_rule(hs.GAT_CASES, lambda c: (c.C % 4 == 0, c.H * c.C))
    _dropout_rule(hs.GAT_CASES, lambda c: c.H * c.C if c.concat else c.C)
    assert {c.concat for c in hs.GAT_CASES} == {True, False}
    lanes = {(4 if c.C % 4 == 0 else 1, hs.pick_lpr(c.H * c.C, 4 if c.C % 4 == 0 else 1)) for c in hs.GAT_CASES}
    assert lanes == {(v, l) for v in (1, 4) for l in (8, 16, 32, 64)}       # <1, 64> and <4, 8> among them
    rect = {c.struct for c in hs.GAT_CASES if hs.structures()[c.struct][0] != hs.structures()[c.struct][1]}
    assert {"wide", "tall", "one_row", "one_col", "edge_empties"} <= rect


@pytest.mark.parametrize("c", hs.GAT_CASES, ids=lambda c: c.id)
def test_gat_reference_is_finite_and_clear_of_the_kinks(c):
    inp = hs.gat_inputs(c)
    width = c.H * c.C if c.concat else c.C
    y, grads, logit_margin, relu_margin = hs.gat_reference(c, inp, hs.host_mask((inp["n_dst"], width), c.p, 1))
    assert y.shape == (inp["n_dst"], width) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert logit_margin >= hs.LOGIT_MARGIN and relu_margin >= hs.RELU_MARGIN


# ---- family 3 -----------------------------------------------------------------------------------------------------------------------
def test_hattn_case_list_covers_the_dispatcher():
    _sweep_rule(hs.HATTN_CASES, lambda c: (c.C % 4 == 0, c.H * c.C))
    _dropout_rule(hs.HATTN_CASES, lambda c: c.H * c.C if c.concat else c.C)
    assert {c.concat for c in hs.HATTN_CASES} == {True, False} and {c.act for c in hs.HATTN_CASES} == {None, "relu", "elu"}
    assert {c.p_attn > 0 for c in hs.HATTN_CASES} == {True, False}
    assert any(c.p_attn == 0.3 for c in hs.HATTN_CASES) and any(c.p_attn == 0.5 for c in hs.HATTN_CASES)
    assert {hs.hattn_packets(c.H, c.C) for c in hs.HATTN_CASES} == {(1, 1), (1, 2), (1, 4), (1, 8), (1, 16), (4, 1), (4, 2), (4, 4)}


@pytest.mark.parametrize("c", hs.HATTN_CASES, ids=lambda c: c.id)
def test_hattn_reference_is_finite_and_clear_of_the_kinks(c):
    inp = hs.hattn_inputs(c)
    width = c.H * c.C if c.concat else c.C
    nnz = inp["ei"].shape[1]
    y, grads, logit_margin, relu_margin = hs.hattn_reference(c, inp, hs.host_mask((nnz, c.H), c.p_attn, 2) if nnz else None,
                                                             hs.host_mask((inp["n_v"], width), c.p, 1))
    assert y.shape == (inp["n_v"], width) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert logit_margin >= hs.LOGIT_MARGIN and relu_margin >= hs.RELU_MARGIN
    deg = np.bincount(inp["ei"][0].numpy(), minlength=inp["n_v"])
    iso = torch.from_numpy(deg == 0)
    if bool(iso.any()) and c.p == 0:                                       # an isolated vertex leaves with act(bias) alone
        import hcha_attn_oracle
        want = hcha_attn_oracle.act_fn(inp["b"], c.act).expand(int(iso.sum()), -1)
        torch.testing.assert_close(y[iso], want, rtol=0, atol=1e-12)   # (elu of a strided against a contiguous row: last-bit differences)


# ---- family 4 -----------------------------------------------------------------------------------------------------------------------
def test_uni_case_lists_cover_the_dispatchers():
    _sweep_rule(hs.UNIGNN_CASES, lambda c: (c.d % 4 == 0, c.d))
    _sweep_rule(hs.UNIGAT_CASES, lambda c: (c.C % 4 == 0, c.H * c.C))
    _sweep_rule(hs.UNIGCN_CASES, lambda c: (c.d % 4 == 0, c.d))
    _dropout_rule(hs.UNIGNN_CASES, lambda c: c.d)
    for cases, width in ((hs.UNIGNN_CASES, lambda c: c.d), (hs.UNIGAT_CASES, lambda c: c.H * c.C), (hs.UNIGCN_CASES, lambda c: c.d)):
        assert {c.variant for c in cases} == {None, 1, 2}
        assert all(width(c) <= 256 for c in cases if c.variant == 2)
        flat = {hs.pick_lpr(width(c), 4) for c in cases if c.variant == 2 and hs.uni_fused(width(c), getattr(c, "C", None))
                and c.struct in ("flat50", "lengths")}
        assert flat == {8, 16, 32, 64}                                     # the short-row kernel at every lane-group width
        assert any(256 < width(c) <= 512 and width(c) % 4 == 0 for c in cases)   # two packets per lane
    assert {(c.use_norm, c.self_term) for c in hs.UNIGNN_CASES} == {(a, b) for a in (True, False) for b in ("none", "float", "tensor")}
    assert any(c.H * c.C > 256 and 256 % c.C for c in hs.UNIGAT_CASES)     # a head that straddles the two packets
    assert all(d > 256 for _, d in hs.UNI_VARIANT_ERRORS)


@pytest.mark.parametrize("c", hs.UNIGNN_CASES, ids=lambda c: c.id)
def test_unignn_reference_is_finite_and_clear_of_the_kinks(c):
    inp = hs.unignn_inputs(c)
    y, grads, t, margin = hs.unignn_reference(c, inp, hs.host_mask((inp["n_v"], c.d), c.p, 1))
    assert y.shape == (inp["n_v"], c.d) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values() if g is not None)
    assert margin >= hs.RELU_MARGIN
    if "zero-rows" in c.id and inp["n_v"] > 1:
        deg = np.bincount(inp["ei"][0].numpy(), minlength=inp["n_v"])
        assert (deg == 0).any() and float(t[torch.from_numpy(deg == 0)].abs().max()) == 0.0 and bool((y[torch.from_numpy(deg == 0)] == 0).all())


@pytest.mark.parametrize("c", hs.UNIGAT_CASES, ids=lambda c: c.id)
def test_unigat_reference_is_finite(c):
    xe, ae, grads = hs.unigat_reference(c, hs.unigat_inputs(c))
    assert all(bool(torch.isfinite(t).all()) for t in (xe, ae, *grads.values()))


@pytest.mark.parametrize("c", hs.UNIGCN_CASES, ids=lambda c: c.id)
def test_unigcn_reference_is_finite(c):
    xi, grads = hs.unigcn_reference(c, hs.unigcn_inputs(c))
    assert all(bool(torch.isfinite(t).all()) for t in (xi, *grads.values()))


# ---- family 5 -----------------------------------------------------------------------------------------------------------------------
def test_han_case_list_covers_the_dispatcher():
    full = [c for c in hs.HAN_CASES if not c.block]
    _sweep_rule(full, lambda c: (c.C % 4 == 0, c.H * c.C))
    _dropout_rule(hs.HAN_CASES, lambda c: c.H * c.C)
    blocks = {c.struct for c in hs.HAN_CASES if c.block}
    assert blocks == {n for n in hs.structures() if hs.han_block_ok(n)} and {"wide", "one_row", "empty", "lengths"} <= blocks
    assert set(hs.HAN_BLOCK_ERRORS) == {"one_col", "edge_empties", "tall"}
    for name in hs.structures():                                           # every node / target has an incoming edge, as the docs ask
        for block in ((False, True) if hs.han_block_ok(name) else (False,)):
            n_src, n_dst, src, dst = hs.han_edges(name, block)
            assert int(torch.bincount(dst, minlength=n_dst).min()) >= 1 and int(src.max()) < n_src


@pytest.mark.parametrize("c", hs.HAN_CASES, ids=lambda c: c.id)
def test_han_reference_is_finite_and_clear_of_the_kink(c):
    inp = hs.han_inputs(c)
    y, grads, logit_margin = hs.han_reference(c, inp, hs.host_mask((inp["src"].numel(), c.H), c.p, 3))
    assert y.shape == (inp["n_dst"], c.H * c.C) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values())
    assert logit_margin >= hs.LOGIT_MARGIN


# ---- family 6 -----------------------------------------------------------------------------------------------------------------------
def test_clique_case_list_covers_the_dispatcher():
    live = [n for n in hs.structures() if n not in hs.CLIQUE_NO_PAIR]
    by = {}
    for c in hs.CLIQUE_CASES:
        by.setdefault(c.struct, set()).add(c.d)
    for name in live:
        assert any(d % 4 == 0 for d in by[name]) and any(d % 4 for d in by[name]), name
    for name in ("edge_empties", "lengths"):
        assert by[name] >= set(hs.VEC_WIDTHS) | set(hs.SCALAR_WIDTHS)
    _dropout_rule(hs.CLIQUE_CASES, lambda c: c.d)
    assert {c.act for c in hs.CLIQUE_CASES} == {None, "relu", "elu"}
    for name in hs.structures():                                           # the asserted errors are exactly the lists without a pair
        assert (hs.clique_adjacency(name) is None) == (name in hs.CLIQUE_NO_PAIR), name
    sizes = np.bincount(hs.structures(hs.LOO_LONG_T)["lengths"][2][1])
    assert {hs.LOO_LONG_T - 1, hs.LOO_LONG_T, hs.LOO_LONG_T + 1} <= set(sizes.tolist())     # both sides of the workgroup kernel's threshold


@pytest.mark.parametrize("c", hs.CLIQUE_CASES, ids=lambda c: c.id)
def test_clique_reference_is_finite_and_clear_of_the_kink(c):
    inp = hs.clique_inputs(c)
    y, grads, margin = hs.clique_reference(c, inp, hs.host_mask((inp["n_v"], c.d), c.p, 1))
    assert y.shape == (inp["n_v"], c.d) and bool(torch.isfinite(y).all())
    assert all(bool(torch.isfinite(g).all()) for g in grads.values()) and margin >= hs.RELU_MARGIN


def test_han_gel_slack_is_the_sum_model_of_the_reference():
    """The one widened tolerance (hop_structures.HAN_GEL_SLACK): finite, large only at the hub source whose 1500 terms cancel, and the
    float64 gradient there is indeed ~0 against terms of O(1)."""
    (c,) = [c for c in hs.HAN_CASES if c.id in hs.HAN_GEL_SLACK]
    inp = hs.han_inputs(c)
    slack = hs.han_gel_slack(c, inp, None)
    _, grads, _ = hs.han_reference(c, inp, None)
    hub = int(torch.bincount(inp["src"]).argmax())
    assert bool(torch.isfinite(slack).all()) and slack.shape == grads["gel"].shape
    assert float(grads["gel"][hub].abs().max()) < 1e-9 and float(slack[hub].min()) > 1e-2
    rest = torch.ones(slack.shape[0], dtype=torch.bool)
    rest[hub] = False
    assert float(slack[rest].max()) < 1e-3


# ---- family 7 -----------------------------------------------------------------------------------------------------------------------
def test_loo_case_list_covers_the_dispatcher():
    live = [n for n in hs.structures() if n not in hs.LOO_DUPLICATES]
    for kind in ("ds", "pma"):
        by = {}
        for c in hs.LOO_CASES:
            if c.kind == kind:
                by.setdefault(c.struct, set()).add(c.H * c.C)
        assert set(by) == set(live) and all(len(v) >= 2 for v in by.values())
        for name in ("edge_empties", "lengths"):
            assert by[name] >= set(hs.VEC_WIDTHS)
    assert {(c.aggr, c.normtype) for c in hs.LOO_CASES if c.kind == "ds"} == {(a, n) for a in ("add", "mean") for n in ("all_one", "deg_half_sym")}
    assert {c.H for c in hs.LOO_CASES if c.kind == "pma"} == {1, 2, 4, 8}
    for name in hs.structures():                                           # the asserted errors are exactly the lists with a repeated pair
        _, _, ei = hs.structures()[name]
        repeated = len(set(zip(ei[0].tolist(), ei[1].tolist()))) != ei.shape[1]
        assert repeated == (name in hs.LOO_DUPLICATES), name
    sizes = hs.loo_expansion("lengths")["ei"][1].bincount().tolist()
    assert {hs.LOO_LONG_T - 1, hs.LOO_LONG_T, hs.LOO_LONG_T + 1, 1, 2} <= set(sizes)       # singletons, pairs, both sides of the threshold


@pytest.mark.parametrize("c", hs.LOO_CASES, ids=lambda c: c.id)
def test_loo_reference_is_finite_and_clear_of_the_kink(c):
    inp = hs.loo_inputs(c)
    assert float(inp["ax"].abs().min()) >= hs.LOGIT_MARGIN and (inp["ay"].numel() == 0 or float(inp["ay"].abs().min()) >= hs.LOGIT_MARGIN)
    if c.kind == "ds":
        A, B, terms_e, terms_v = hs.loo_matrices(c.struct, c.aggr, c.normtype)
        for t in (A @ inp["x"], A.t() @ inp["G_e"], B @ inp["y"], B.t() @ inp["G_v"]):
            assert bool(torch.isfinite(t).all())
        r = hs.loo_expansion(c.struct)
        assert A.shape == (r["nnz"], r["n_v"]) and B.shape == (r["n_dst"], r["nnz"])
    else:
        for out, gV, ga in hs.loo_pma_reference(c, inp).values():
            assert all(bool(torch.isfinite(t).all()) for t in (out, gV, ga))


# ---- the test hook -----------------------------------------------------------------------------------------------------------------------
def test_hconv_variant_hook_keeps_the_csrs_choice_and_passes_an_override_on():
    from allset_amd import ops
    from allset_amd._lib import AllSetHipError
    rowptr = torch.arange(0, 3 * 20001, 3, dtype=torch.int32)
    big = ops.CSR(rowptr, torch.zeros(60000, dtype=torch.int32), None, 20000, 20000, 3)       # > 16384 rows, mean degree 3
    small = ops.CSR(rowptr[:51], torch.zeros(150, dtype=torch.int32), None, 50, 50, 3)
    assert ops._hconv_variant(big, 20000, True, None) == big.variant("segreduce", 20000) == 2
    assert ops._hconv_variant(big, 20000, False, None) == 1                                   # rows the short-row kernel cannot take
    assert ops._hconv_variant(small, 50, True, None) == small.variant("segreduce", 50) == 1
    for csr, n in ((big, 20000), (small, 50)):
        assert ops._hconv_variant(csr, n, True, 1) == 1 and ops._hconv_variant(csr, n, False, 2) == 2   # as given: the C entry refuses
    with pytest.raises(AllSetHipError, match="variant must be None, 1 or 2"):
        ops._hconv_variant(small, 50, True, 0)


# ---- the short-row kernels of segreduce.hip / pma.hip (tests/test_gpu_flat_walk.py) -------------------------------------------------
def test_flat_walk_widths_take_every_lane_group_and_the_split_structure_has_both_kinds_of_rows():
    from allset_amd import ops
    assert hs.FLAT_WIDTHS == (4, 12, 32, 36, 64, 68, 128, 132, 256) and tuple(hs.FLAT_PMA_HC) == hs.FLAT_WIDTHS
    assert {hs.pick_lpr(d, 4) for d in hs.FLAT_WIDTHS} == {8, 16, 32, 64}
    assert {hs.pick_lpr(d, 8) for d in hs.FLAT_WIDTHS if d % 8 == 0} == {8, 16, 32}      # bf16: 8 elements per 16-byte packet
    assert all(H * C == d and C % 4 == 0 for d, (H, C) in hs.FLAT_PMA_HC.items())
    n_src, n_dst, ei = hs.structures()[hs.FLAT_SPLIT_STRUCT]
    deg = torch.from_numpy(_deg(ei, n_dst, 1))
    rowptr = torch.zeros(n_dst + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0)
    col = torch.zeros(int(deg.sum()), dtype=torch.int32)
    sp = ops.size_split(rowptr, col, n_dst, int(deg.max()), threshold=hs.CSR_LONG_T)
    assert sp is not None and sp.long_ids.tolist() == [int(deg.argmax())] and sp.short_ids.numel() == n_dst - 1
    short_deg = (sp.rowptr_short[1:] - sp.rowptr_short[:-1]).tolist()
    assert max(short_deg) == hs.CSR_LONG_T and 0 in short_deg and sp.short_ids.tolist() != list(range(n_dst - 1))   # ids are not the identity


@pytest.mark.parametrize("name", list(hs.structures()))
def test_flat_walk_references_are_finite_and_clear_of_the_leaky_relu_kink(name):
    d = hs.FLAT_WIDTHS[list(hs.structures()).index(name) % len(hs.FLAT_WIDTHS)]
    inp = hs.flat_segreduce_inputs(name, d)
    for aggr, weighted in (("add", False), ("mean", False), ("add", True)):
        ref = hs.flat_segreduce_reference(inp, inp["x"], aggr, weighted)
        assert ref.shape == (inp["n_dst"], d) and bool(torch.isfinite(ref).all())
    H, C = hs.FLAT_PMA_HC[d]
    for transposed in (False, True):
        pin = hs.flat_pma_inputs(name, H, C, transposed)
        assert float(pin["alpha"].abs().min()) >= hs.LOGIT_MARGIN
        out, m, l, gV, ga = hs.flat_pma_reference(pin)
        assert out.shape == (pin["n_dst"], d) and m.shape == l.shape == (pin["n_dst"], H)
        assert gV.shape == (pin["n_src"], d) and ga.shape == (pin["n_src"], H)
        assert all(bool(torch.isfinite(t).all()) for t in (out, m, l, gV, ga))
        got = torch.from_numpy(_deg(pin["ei"].numpy(), pin["n_dst"], 1)) > 0
        assert torch.equal(l.min(dim=1).values >= 1.0, got) and torch.equal(l.max(dim=1).values > 0, got)   # l >= 1 where a row has members


def test_flat_walk_galpha_slack_stays_far_below_one_incidence_at_every_width():
    """The allowance of hop_structures.FLAT_GALPHA_SLACK: non-zero at the hub source alone, between the family rule's 1e-4 and 5e-2
    at every width, and at least 4 times smaller than what the smallest single incidence contributes to D (so a dropped or doubled
    incidence cannot hide in it)."""
    from oracle import allset_oracle
    for name in hs.FLAT_GALPHA_SLACK:
        for d, (H, C) in hs.FLAT_PMA_HC.items():
            pin = hs.flat_pma_inputs(name, H, C, True)
            ga = hs.flat_pma_reference(pin)[4]
            slack = hs.flat_pma_galpha_slack(pin)
            src, dst = pin["ei"]
            hub = int(src[0])
            assert len(set(src.tolist())) == 1 and float(ga.abs().max()) < 1e-12
            assert 1e-4 < float(slack[hub].min()) and float(slack[hub].max()) < 5e-2, (d, slack[hub])
            assert float(slack.sum() - slack[hub].sum()) == 0.0
            p = allset_oracle.segment_softmax(torch.nn.functional.leaky_relu(pin["alpha"][src], 0.2), dst, pin["n_dst"])
            out = hs.flat_pma_reference(pin)[0].view(pin["n_dst"], H, C)
            delta = (out * pin["G"].view(pin["n_dst"], H, C)).sum(-1)
            one = (p * delta[dst].abs() * torch.where(pin["alpha"][src] > 0, 1.0, 0.2))
            print(d, "slack", slack[hub].tolist(), "median single-incidence term", one.median(dim=0).values.tolist())
            assert bool((4 * slack[hub] < one.median(dim=0).values).all()), d
