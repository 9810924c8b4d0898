"""CPU: the cases tests/test_gpu_bf16_dense.py runs, vouched for from float64 alone -- every table is representable in its storage
type, the exact tables are exact in fp32 in any order and land on bf16 ties often enough to tell round-to-nearest-even from anything
else, the width and shape lists reach every instantiation the launchers of csrc/dense.hip can select, the relu / dropout cases keep
their unsure elements under the cap, and the acceptance rules reject the wrong kernels on the cases themselves.  Cases, tables,
references and rules are imported from tests/bf16_dense_cases.py, the module the GPU file imports them from."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_dense_cases as dc  # noqa: E402

N_DISC = 37                                            # the row count the discrimination figures are measured at


def _bf16_exact(t):
    return bool((t.float().bfloat16().double() == t).all())


def _f32_exact(t):
    return bool((t.float().double() == t).all())


# ---- representability ------------------------------------------------------------------------------------------------------------------
def test_layer_norm_tables_are_bf16_values_with_both_zeros():
    for d in dc.LN_WIDTHS:
        for n in dc.ln_rows(d):
            t = dc.ln_inputs(n, d)
            assert all(_bf16_exact(v) for v in t.values())
            x = t["x"]
            zeros = x == 0
            neg = zeros & torch.signbit(x)
            assert int(neg.sum()) >= 1 and int((zeros & ~neg).sum()) >= 1, (n, d)
            assert bool((x.to(torch.bfloat16).double() == x).all()) and bool(torch.signbit(x.to(torch.bfloat16))[neg].all())
    for d, H in dc.LN_PMA_SHAPES:
        m, l, empty = dc.pma_ml(dc.LN_PMA_ROWS, H)
        assert _f32_exact(m) and _f32_exact(l) and int(empty.sum()) == 3
        assert bool((l[empty] == 0).all()) and bool((l[~empty] >= 1).all())


def test_weight_gradient_tables_are_representable_and_the_exact_ones_exact():
    """|ga|, |u| <= 8: a partial sum of ANY order is bounded by 64 n <= 64000 < 2^24, an integer, exact in fp32."""
    assert 64 * max(dc.WG_ROWS_LIST) < 2 ** 24
    for c in dc.WG_FULL_CASES + dc.WG_TILED_CASES:
        ga, u, g4 = dc.wgrad_tables(c.n, c.O, c.I, "exact")
        for t in (ga, u, g4):
            assert _bf16_exact(t) and bool((t == t.round()).all()) and float(t.abs().max()) <= 8
        if c.n >= 33:
            assert float(ga.min()) == -8 and float(ga.max()) == 8
        for ref in dc.wgrad_reference(ga, u, None, g4):
            assert bool((ref == ref.round()).all()) and float(ref.abs().max()) < 2 ** 24 and _f32_exact(ref)
        ga, u, g4 = dc.wgrad_tables(c.n, c.O, c.I, "general")
        assert _bf16_exact(ga) and _bf16_exact(u) and _f32_exact(g4) and not _bf16_exact(g4)
    for P, M, stride in dc.REDUCE_CASES:
        part = dc.reduce_partials_table(P, stride, "exact")
        assert _f32_exact(part) and bool((part == part.round()).all()) and 4000 * P < 2 ** 24
        assert _f32_exact(dc.reduce_partials_table(P, stride, "general"))


def test_adam_tables_are_representable_and_span_the_scales():
    for bf16 in (True, False):
        p, g, m, v = dc.adam_state(4097, bf16, "case")
        for t in (p, g, m, v):
            assert _bf16_exact(t) if bf16 else _f32_exact(t)
        assert float(g.abs().min()) < 2e-4 and float(g.abs().max()) > 50 and float(v.min()) > 0 and float(v.min()) < 2e-8 and float(v.max()) > 50
        assert int((g > 0).sum()) > 1500 and int((g < 0).sum()) > 1500 and int((m < 0).sum()) > 1500
        wd = max(dc.ADAM_WD)
        assert bool(((g + wd * p).abs() >= 0.5 * (wd * p).abs()).all())            # the product wd * p is budgeted against |g + wd p|
    lr, b1, b2, eps, wd = dc.adam_hyper32(wd=0.01, **dc.ADAM_HYPER)
    assert np.float32(1) - np.float32(b1) == 1 - b1 and np.float32(1) - np.float32(b2) == 1 - b2      # 1 - beta is exact in fp32


# ---- instantiation coverage ------------------------------------------------------------------------------------------------------------
def test_layer_norm_cases_reach_every_instantiation():
    assert [dc.ln_bf16_lpr(d) for d in dc.LN_WIDTHS] == [8, 8, 8, 16, 16, 32, 32, 64, 64, 64]
    full = {d for d in dc.LN_WIDTHS if d == 8 * dc.ln_bf16_lpr(d)}
    assert {dc.ln_bf16_lpr(d) for d in full} == set(dc.LN_LPRS) == {dc.ln_bf16_lpr(d) for d in set(dc.LN_WIDTHS) - full}
    assert (dc.ln_rows_per_block(64), dc.ln_rows_per_block(512)) == (128, 16)
    for d in dc.LN_WIDTHS:                                                        # a forward tail workgroup with clamped loads
        assert dc.ln_rows(d)[-1] == dc.ln_res_rows(d)[-1] == dc.ln_rows_per_block(d) + 1
    assert {(dc.ln_bf16_lpr(c.d), c.relu_in, c.p > 0) for c in dc.LN_CASES} == {(l, r, p) for l in dc.LN_LPRS for r in (False, True) for p in (False, True)}
    n = dc.ln_grid_stride_rows(dc.LN_BWD_PARTIALS_CAP)
    assert n == 8193 and dc.ln_bwd_partials(n, dc.LN_GRID_STRIDE_D) * dc.ln_groups(dc.LN_GRID_STRIDE_D) == n - 1
    assert all(c.ld % 8 == 0 and c.ld > c.d for c in dc.LN_LD_CASES)
    assert dc.ln_res_instantiations() == dc.ln_res_all_instantiations() and len(dc.ln_res_all_instantiations()) == 20
    for lpr in dc.LN_LPRS:                                                        # colb and relu_out on and off with every instantiation
        for r in (False, True):
            for dr in (False, True):
                got = {(c.has_colb, c.relu_out) for c in dc.LN_RES_CASES if (dc.ln_bf16_lpr(c.d), c.has_res, c.p > 0) == (lpr, r, dr)}
                assert len(got) == 4
    assert [dc.pma_lanes_per_head(d, H) for d, H in dc.LN_PMA_SHAPES] == [1, 1, 8, 8, 64, 4]
    assert [8 * dc.ln_bf16_lpr(d) == d for d, _ in dc.LN_PMA_SHAPES] == [True, False, False, True, True, True]


def test_weight_gradient_cases_reach_every_kernel():
    reached = {dc.wgrad_kernel(c) for c in dc.WG_FULL_CASES + dc.WG_TILED_CASES}
    reached |= {dc.wgrad_kernel(dc.WgCase(c.id, c.n, c.O, c.I, c.O, c.I), c.bits, c.aux) for c in dc.WG_EX2_CASES}
    assert reached == dc.wgrad_all_kernels() and len(reached) == 16
    assert dc.wgrad_kernel(dc.WG_TILED_CASES[-1]) == ("tiled",) and dc.wgrad_bf16_full_width(64, 64)
    assert [dc.wgrad_bf16_slices(n, 256, 256) for n in dc.WG_ROWS_LIST] == [1, 1, 1, 2, 4]
    assert [dc.wgrad_bf16_slices(n, 64, 128) for n in dc.WG_ROWS_LIST] == [1, 1, 1, 2, 4]
    assert 1000 % 4 != 0 or -(-1000 // 4) % 32 != 0                               # a ragged last slice
    assert {dc.reduce_is_tree(P, M) for P, M, _ in dc.REDUCE_CASES} == {False, True}
    assert [dc.reduce_is_tree(P, 260) for P in (1, 5, 64, 65, 700)] == [False, False, False, False, True]
    assert sum(1 for P, M, s in dc.REDUCE_CASES if s > M) == 1


def test_adam_sizes_straddle_the_chunk_and_the_table():
    s = dc.adam_sizes(48)
    assert len(s) == 49 and s[3] == 0 and s[2] > 0 and s[4] > 0
    assert {dc.ADAM_CHUNK - 1, dc.ADAM_CHUNK, dc.ADAM_CHUNK + 1, 2 * dc.ADAM_CHUNK + 1, 1} <= set(s)
    assert [t + 1 for t in dc.ADAM_PRE_STEPS] == [1, 2, 10, 1000]


# ---- caps ------------------------------------------------------------------------------------------------------------------------------
def test_unsure_elements_stay_under_the_cap():
    """An element is unsure where the float64 pre-activation is within 1e-3 of zero (relu_out or dropout cases only): at most 0.5 % of
    any case (measured: at most 0.40 %, one element of the smallest cases)."""
    worst = 0.0
    for c in dc.LN_RES_CASES:
        t = dc.ln_inputs(c.n, c.d)
        r = dc.ln_reference(t["x"], t["gamma"], t["beta"], None, False, t["colb"] if c.has_colb else None, t["res"] if c.has_res else None)
        u = dc.unsure_elements(r["pre"], c.relu_out, c.p)
        assert (c.relu_out or c.p > 0) or not bool(u.any())
        worst = max(worst, float(u.double().mean()))
        assert float(u.double().mean()) <= dc.UNSURE_CAP, c.id
    for c in dc.LN_CASES + dc.LN_LD_CASES:
        t = dc.ln_inputs(c.n, c.d)
        r = dc.ln_reference(t["x"], t["gamma"], t["beta"], None, c.relu_in)
        u = dc.unsure_elements(r["pre"], False, c.p)
        worst = max(worst, float(u.double().mean()))
        assert float(u.double().mean()) <= dc.UNSURE_CAP, c.id
    print(f"unsure elements: at most {worst:.4%} of a case")


@pytest.mark.parametrize("n", dc.WG_CENSUS_ROWS)
def test_exact_weight_gradients_hit_ties_and_inexact_values(n):
    """Over the nine full-width shapes at n = 257 and n = 1000: at least 10 % of the exact-table outputs are bf16 ties, at least 20 %
    are inexact in bf16 and at least 10 % differ from truncation (measured at n = 257: 21 / 30 / 15 %; at n = 1000: 22 / 52 / 26 %)."""
    ties = inexact = trunc = total = 0
    for O in dc.WG_FULL_WIDTHS:
        for I in dc.WG_FULL_WIDTHS:
            ga, u, _ = dc.wgrad_tables(n, O, I, "exact")
            ref = dc.wgrad_reference(ga, u)[0]
            r = dc.bf16_round(ref)
            t, ix, tr = (r - ref).abs() == 0.5 * dc.ulp_bf16(ref), r != ref, dc.truncate_bf16(ref) != r
            t &= ref != 0
            for share, floor in ((t, 0.10), (ix, 0.20), (tr, 0.10)):
                assert float(share.double().mean()) >= floor, (n, O, I)
            ties, inexact, trunc, total = ties + int(t.sum()), inexact + int(ix.sum()), trunc + int(tr.sum()), total + ref.numel()
    print(f"n {n}: ties {ties / total:.3f}, inexact {inexact / total:.3f}, differ from truncation {trunc / total:.3f} of {total}")


# ---- discrimination --------------------------------------------------------------------------------------------------------------------
def _ln_disc_refs():
    for d in dc.LN_WIDTHS:
        t = dc.ln_inputs(N_DISC, d)
        yield d, t, dc.ln_reference(t["x"], t["gamma"], t["beta"], t["G"])


def _share(bad):
    return float(bad.double().mean())


def test_rule_rejects_truncation_of_layer_norm_outputs_and_gradients():
    """Per width at n = 37 the rule accepts the correctly rounded y and gx everywhere and rejects the truncated ones (measured: 41 to
    43 % of y, 40 to 43 % of gx); asserted: half."""
    for d, t, r in _ln_disc_refs():
        for k, floor in (("y", 0.41), ("gx", 0.40)):
            ref = r[k]
            assert bool(dc.within_one_rounding(dc.bf16_round(ref), ref).all())
            bad = ~dc.within_one_rounding(dc.truncate_bf16(ref), ref)
            print(f"d {d} {k}: truncation rejected on {_share(bad):.3f}")
            assert _share(bad) >= 0.5 * floor, (d, k)


def test_rule_rejects_a_bf16_normalised_row():
    """x_hat rounded to bf16 before the affine: rejected on 22 to 24 % of the outputs (measured per width at n = 37); asserted: half."""
    for d, t, r in _ln_disc_refs():
        xh = dc.bf16_round((t["x"] - r["mean"][:, None]) * r["rstd"][:, None])
        bad = ~dc.within_one_rounding(dc.bf16_round(xh * t["gamma"] + t["beta"]), r["y"])
        print(f"d {d}: bf16 x_hat rejected on {_share(bad):.3f}")
        assert _share(bad) >= 0.5 * 0.22, d


def test_rule_rejects_a_bf16_accumulator_for_the_parameter_gradients():
    """dgamma summed over 37 rows with the accumulator rounded to bf16 after every row: rejected on 64 to 78 % of the columns
    (measured per width); gW over 257 rows of the general tables at 64 x 64: 89 %; asserted: half."""
    for d, t, r in _ln_disc_refs():
        xh = (t["x"] - r["mean"][:, None]) * r["rstd"][:, None]
        acc = torch.zeros(d, dtype=dc.D64)
        for i in range(N_DISC):
            acc = dc.bf16_round(acc + t["G"][i] * xh[i])
        assert bool(dc.within_one_rounding(dc.bf16_round(r["dgamma"]), r["dgamma"]).all())
        bad = ~dc.within_one_rounding(acc, r["dgamma"])
        print(f"d {d}: bf16 accumulator rejected on {_share(bad):.3f} of dgamma")
        assert _share(bad) >= 0.5 * 0.64, d
        assert bool(bad.any())
    ga, u, _ = dc.wgrad_tables(257, 64, 64, "general")
    ref = dc.wgrad_reference(ga, u)[0]
    acc = torch.zeros(64, 64, dtype=dc.D64)
    for i in range(257):
        acc = dc.bf16_round(acc + ga[i][:, None] * u[i][None, :])
    assert bool(dc.within_one_rounding(dc.bf16_round(ref), ref).all())
    bad = ~dc.within_one_rounding(acc, ref)
    print(f"bf16 accumulator rejected on {_share(bad):.3f} of gW")
    assert _share(bad) >= 0.5 * 0.889


def _adam_emulated(p, g, m, v, t, wd, bf16, flaw=None):
    """The kernel's arithmetic in numpy float32, statement by statement, with one flaw at a time."""
    f = np.float32
    lr, b1, b2, eps, wd = (f(x) for x in dc.adam_hyper32(wd=wd, **dc.ADAM_HYPER))
    pv, gv0, mo, vo = (x.numpy().astype(f) for x in (p, g, m, v))
    rb = lambda a: torch.from_numpy(np.asarray(a, dtype=f)).bfloat16().float().numpy()
    gv = gv0 + wd * pv
    if flaw == "bf16-intermediates":
        mv = rb(rb(b1 * mo) + rb((f(1) - b1) * gv))
        vv = rb(rb(b2 * vo) + rb(rb((f(1) - b2) * gv) * gv))
    else:
        mv = b1 * mo + (f(1) - b1) * gv
        vv = b2 * vo + (f(1) - b2) * gv * gv
    bc1, bc2 = f(1) - np.power(b1, f(t), dtype=f), f(1) - np.power(b2, f(t), dtype=f)
    if flaw == "no-bias-correction":
        bc1 = bc2 = f(1)
    step, isb = lr / bc1, f(1) / np.sqrt(bc2)
    den = np.sqrt(vv * isb * isb + eps) if flaw == "eps-inside" else np.sqrt(vv) * isb + eps
    pn = pv - step * mv / den
    st = (lambda a: torch.from_numpy(a).bfloat16().double()) if bf16 else (lambda a: torch.from_numpy(a).double())
    return dict(p=st(pn), m=st(mv), v=st(vv))


@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_adam_bounds_accept_the_fp32_arithmetic_and_reject_the_flawed_kernels(bf16):
    """The kernel's statements in numpy float32 pass the three bounds on every element, at every pre-step counter and weight decay
    of the cases.  Rejected (measured over 4097 elements, bf16 / fp32 storage; asserted: half):
      * moments updated from bf16-rounded intermediates: exp_avg 21 % / 100 %, exp_avg_sq 14 % / 99.9 % at every counter (in bf16
        storage the flaw hides behind the final rounding wherever one term dominates the sum);
      * no bias correction: the parameter on 81 % / 99 % at t = 1, 2 and 10, and on 71 % / 99 % at t = 1000 (1 - b2^t = 0.63);
      * eps added inside the square root, sqrt(v / (1 - b2^t) + eps): the parameter on 6 % / 17 % at t = 1000 -- at t <= 10 the
        corrected second moment is above 1e-6 and eps = 1e-8 inside the root moves nothing, so it is asserted at t = 1000 only;
      * a kernel that does nothing: the parameter 70 % / 99 %, exp_avg 99.8 % / 100 %, exp_avg_sq 53 % / 99.9 %."""
    floors = {"bf16-intermediates": {"m": (0.21, 1.0), "v": (0.137, 0.999)},
              "no-bias-correction": {1: (0.80, 0.99), 2: (0.80, 0.99), 10: (0.80, 0.99), 1000: (0.71, 0.98)},
              "eps-inside": {1000: (0.06, 0.17)}, "nothing": {"p": (0.70, 0.98), "m": (0.99, 1.0), "v": (0.52, 0.99)}}
    p, g, m, v = dc.adam_state(4097, bf16, "case")
    col = 0 if bf16 else 1
    for pre in dc.ADAM_PRE_STEPS:
        t = pre + 1
        for wd in dc.ADAM_WD:
            ref = dc.adam_reference(p, g, m, v, t, wd=wd, **dc.ADAM_HYPER)
            good = _adam_emulated(p, g, m, v, t, wd, bf16)
            for k in ("m", "v", "p"):
                assert bool(dc.adam_within(good[k], ref, k, bf16).all()), (t, wd, k)
            bad = _adam_emulated(p, g, m, v, t, wd, bf16, "bf16-intermediates")
            for k in ("m", "v"):
                share = _share(~dc.adam_within(bad[k], ref, k, bf16))
                print(f"t {t} wd {wd} bf16 intermediates: {k} rejected on {share:.3f}")
                assert share >= 0.5 * floors["bf16-intermediates"][k][col]
            for flaw in ("no-bias-correction", "eps-inside"):
                share = _share(~dc.adam_within(_adam_emulated(p, g, m, v, t, wd, bf16, flaw)["p"], ref, "p", bf16))
                print(f"t {t} wd {wd} {flaw}: p rejected on {share:.3f}")
                if t in floors[flaw]:
                    assert share >= 0.5 * floors[flaw][t][col], (flaw, t, wd)
    # a kernel that did nothing fails all three
    ref = dc.adam_reference(p, g, m, v, 2, wd=0.0, **dc.ADAM_HYPER)
    for k, old in (("p", p), ("m", m), ("v", v)):
        assert _share(~dc.adam_within(old, ref, k, bf16)) >= 0.5 * floors["nothing"][k][col]


def test_pma_statistics_reference_marks_the_empty_rows():
    d, H = dc.LN_PMA_SHAPES[2]
    t = dc.ln_inputs(dc.LN_PMA_ROWS, d, "pma")
    m, l, empty = dc.pma_ml(dc.LN_PMA_ROWS, H)
    st = dc.pma_stats_dense_reference(t["x"], t["G"], m, l, H)
    assert bool((st[empty][..., 0] == dc.FLT_MAX).all()) and bool(torch.isfinite(st[~empty]).all()) and float(st[~empty][..., 0].abs().max()) < 10
    assert torch.allclose(st[..., 1].sum(1), (t["x"] * t["G"]).sum(1), rtol=1e-12, atol=1e-12)
