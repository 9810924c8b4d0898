"""CPU: the cases tests/test_gpu_bf16_aggregate.py runs, vouched for from float64 alone -- the exact tables are exact (in fp32, in any
order) and land on bf16 ties and inexact values often enough to tell round-to-nearest-even from anything else; the acceptance rule
accepts one rounding and rejects truncation and a bf16 accumulator; the width and shape lists reach every (VEC, LPR) pair of the bf16
instantiations.  Cases, tables and the rule are imported from tests/bf16_cases.py, the module the GPU file imports them from."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_cases as bc  # noqa: E402
import hop_structures as hs  # noqa: E402

WIDTHS = sorted({w.d for w in bc.SEG_WIDTHS})


def _bf16_exact(t):
    return bool((t.float().bfloat16().double() == t).all())


def test_structure_is_what_the_cases_say():
    n_src, n_dst, ei = bc.structure()
    assert (n_src, n_dst) == (300, 40) and ei.dtype == np.int64 and ei.shape[0] == 2 and ei.shape[1] < 3000
    lengths = np.bincount(ei[1], minlength=n_dst)
    assert tuple(lengths[:15]) == (0, 0, 1, 2, 3, 17, 63, 64, 65, 127, 128, 130, 300, 0, 1) and lengths[15:].max() < 8
    assert 0 <= ei[0].min() and ei[0].max() < n_src
    assert not np.array_equal(ei[1], np.sort(ei[1]))                              # edge-list order is not CSR order
    big = ei[0][ei[1] == 12]
    assert len(set(big.tolist())) < 300                                           # duplicate sources inside a row
    for flip in (False, True):
        csr = bc.host_csr(flip)
        rows, cols = (ei[0], ei[1]) if flip else (ei[1], ei[0])
        assert csr.rowptr[0] == 0 and csr.rowptr[-1] == ei.shape[1] and np.all(np.diff(csr.rowptr) >= 0)
        assert np.array_equal(rows[csr.perm], np.repeat(np.arange(csr.n_rows), np.diff(csr.rowptr)))
        assert np.array_equal(cols[csr.perm], csr.col)
        for t in range(csr.n_rows):                                               # stable: ties keep the edge-list order
            assert np.all(np.diff(csr.perm[csr.rowptr[t]:csr.rowptr[t + 1]]) > 0)
    assert (bc.row_lengths(True) == 0).any() and bc.row_lengths(True).max() < 64  # the transposed rows are short, some empty


def test_tables_hold_what_their_storage_types_hold():
    for d in WIDTHS:
        x, xs = bc.exact_table(d), bc.exact_table(d, signed=True)
        assert float(x.min()) == 0 and float(x.max()) == 16 and float(xs.min()) == -8 and float(xs.max()) == 8
        assert bool((x == x.round()).all()) and bool((xs == xs.round()).all())
        assert _bf16_exact(x) and _bf16_exact(xs) and _bf16_exact(bc.general_table(300, d))
    w = bc.exact_weights()
    assert set(w.tolist()) == {0.5, 1.0, 2.0, 4.0}
    gw = bc.general_weights()
    assert bool((gw.float().double() == gw).all()) and float(gw.min()) >= 0.5 and float(gw.max()) < 1.5
    for H in (1, 3, 8):
        a = bc.logits(300, H, "alpha")
        assert bool((a.float().double() == a).all()) and bool(((a * 16) % 2 == 1).all()) and float(a.abs().min()) >= 1 / 16


def _exact_sum_census(weighted):
    """Every exact-table reference survives ``.float()`` unchanged and is a multiple of 0.5; returns (ties, inexact, outputs) of the
    SUM references over the rows of length >= 64, all widths."""
    w = bc.exact_weights() if weighted else None
    lengths = bc.row_lengths()
    long_rows = torch.from_numpy(lengths >= 64)
    assert int(long_rows.sum()) == 6
    ties = inexact = total = 0
    for d in WIDTHS:
        for signed in (False, True):
            x = bc.exact_table(d, signed)
            for reduce in ((bc.SUM,) if not signed else (bc.MAX, bc.MIN)):
                ref, arg = bc.seg_reference(reduce, x, w)
                assert bool((ref.float().double() == ref).all())
                assert bool(((2 * ref) == (2 * ref).round()).all())
                if reduce != bc.SUM:
                    assert _bf16_exact(ref)                                       # an extremum of products k * w, |k| <= 8: <= 4 significant bits
                    assert bool(((arg >= 0) == torch.from_numpy(lengths > 0).view(-1, 1)).all())
        ref, _ = bc.seg_reference(bc.SUM, bc.exact_table(d), w)
        r = ref[long_rows]
        rounded = bc.bf16_round(r)
        tie = (rounded - r).abs() == 0.5 * bc.ulp_bf16(r)
        inexact += int((rounded != r).sum())
        ties += int(tie.sum())
        total += r.numel()
        print(f"d {d} weighted {weighted}: ties per long row {[round(float(v), 3) for v in tie.double().mean(1)]}, inexact "
              f"{[round(float(v), 3) for v in (rounded != r).double().mean(1)]}")
    print(f"weighted {weighted}: ties {ties / total:.3f}, inexact {inexact / total:.3f} of {total} outputs")
    return ties, inexact, total


def test_exact_references_are_exact_in_fp32_and_hit_ties():
    """The partial sums of ANY order are bounded by the sum of the magnitudes, 16 * 4 * 300 < 2^23 halves: exact in fp32.  Over the rows
    of length >= 64 at least 10 % of the sum outputs (the unweighted and the weighted table together; unweighted alone: 22 %, weighted
    alone: 7 % -- a weighted sum is a multiple of 0.5, two more low bits to round away) are exact bf16 ties and at least 50 % of either
    table's are inexact."""
    assert 2 * 16 * 4 * int(bc.row_lengths().max()) < 2 ** 23
    plain, weighted = _exact_sum_census(False), _exact_sum_census(True)
    assert plain[0] + weighted[0] >= 0.10 * (plain[2] + weighted[2])
    assert plain[0] >= 0.10 * plain[2] and weighted[0] >= 0.02 * weighted[2]
    assert plain[1] >= 0.50 * plain[2] and weighted[1] >= 0.50 * weighted[2]


def test_ties_have_neighbours_of_both_parities():
    """Round to nearest EVEN is told from round-half-up and round-half-down only by ties whose lower neighbour is even AND ties whose
    lower neighbour is odd: both kinds occur among the exact sums."""
    ref, _ = bc.seg_reference(bc.SUM, bc.exact_table(128))
    u = bc.ulp_bf16(ref)
    tie = (bc.bf16_round(ref) - ref).abs() == 0.5 * u
    tie &= u > 0
    low = torch.floor(ref[tie] / u[tie])                                         # the lower bf16 neighbour in units of ulp
    assert int((low % 2 == 0).sum()) >= 20 and int((low % 2 == 1).sum()) >= 20
    assert bool((bc.bf16_round(ref)[tie] / u[tie] % 2 == 0).all())             # and torch rounds them to even


def test_ulp_is_the_spacing_of_bf16():
    r = torch.tensor([1.0, 1.99, 2.0, 3.0, 0.75, 300.0, -300.0, 0.0, 2.0 ** -20], dtype=torch.float64)
    want = torch.tensor([2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -8, 2.0, 2.0, 0.0, 2.0 ** -27], dtype=torch.float64)
    assert torch.equal(bc.ulp_bf16(r), want)
    one = torch.tensor([1.0], dtype=torch.bfloat16)
    nxt = (one.view(torch.int16) + 1).view(torch.bfloat16)
    assert float(nxt.double() - 1.0) == float(bc.ulp_bf16(one.double()))


def test_rule_accepts_one_rounding_and_rejects_truncation():
    """Over the general-table references the GPU file applies the rule to (SUM and MEAN, without and with weights, every width) the
    rule accepts ``ref.float().bfloat16()`` everywhere and rejects the truncated value (``bits & 0xffff0000``) on at least 25 % of
    the elements.  Truncation is off by a uniform share of an ulp, so it is rejected on about half of the elements that carry a
    rounding at all (the rule's fp32 terms take 1e-4 * 2^8 + 1e-4 * 2^7 < 4 % of an ulp at |ref| >= 1): at least 40 % of a SUM's
    elements on the rows of length >= 17; empty rows and the unweighted sum of a one-incidence row are bf16 values, where truncation
    changes nothing."""
    total = rejected = 0
    long_rows = torch.from_numpy(bc.row_lengths() >= 17)
    for weighted in (False, True):
        for reduce in (bc.SUM, bc.MEAN):
            n = r = nl = rl = 0
            for d in WIDTHS:
                ref, _ = bc.seg_reference(reduce, bc.general_table(300, d), bc.general_weights() if weighted else None)
                assert bool(bc.within_one_rounding(ref.float().bfloat16(), ref).all())
                trunc = (ref.float().view(torch.int32) & -65536).view(torch.float32)      # bits & 0xffff0000
                assert bool((trunc.bfloat16().float() == trunc).all())
                bad = ~bc.within_one_rounding(trunc, ref)
                n, r, nl, rl = n + bad.numel(), r + int(bad.sum()), nl + bad[long_rows].numel(), rl + int(bad[long_rows].sum())
            print(f"reduce {reduce} weighted {weighted}: truncation rejected on {r / n:.3f} of {n} elements, {rl / nl:.3f} on the long rows")
            assert reduce == bc.MEAN or rl >= 0.40 * nl                          # (a long row's mean is O(0.1): the rule's 1e-4 is a large share of its ulp)
            total, rejected = total + n, rejected + r
            # and on the exact tables (ties round to even)
            ref, _ = bc.seg_reference(reduce, bc.exact_table(128), bc.exact_weights() if weighted else None)
            assert bool(bc.within_one_rounding(ref.float().bfloat16(), ref).all())
    print(f"truncation rejected on {rejected / total:.3f} of {total} elements")
    assert rejected >= 0.25 * total


def test_rule_rejects_a_bf16_accumulator():
    """The same sum with the accumulator rounded to bf16 after every addition.  n roundings of up to 1/2 ulp each walk ~ sqrt(n / 12)
    ulp from the exact sum -- 2.3 ulp at n = 64 -- where the rule allows about 1/2: over the rows of length >= 64 at least half of the
    elements (expected: over 80 %) are rejected, and the result as a whole is."""
    x = bc.general_table(300, 128)
    ref, _ = bc.seg_reference(bc.SUM, x)
    csr = bc.host_csr()
    acc = torch.zeros(csr.n_rows, 128, dtype=torch.bfloat16)
    xb = x.bfloat16()
    for t in range(csr.n_rows):
        a = torch.zeros(128, dtype=torch.bfloat16)
        for j in range(int(csr.rowptr[t]), int(csr.rowptr[t + 1])):
            a = (a.float() + xb[csr.col[j]].float()).bfloat16()
        acc[t] = a
    ok = bc.within_one_rounding(acc, ref)
    long_rows = torch.from_numpy(bc.row_lengths() >= 64)
    frac = float((~ok[long_rows]).double().mean())
    print(f"bf16 accumulator: rejected on {frac:.3f} of the long rows' elements, {float((~ok).double().mean()):.3f} overall")
    assert not bool(ok.all()) and frac >= 0.5
    assert bool(ok[torch.from_numpy(bc.row_lengths() <= 1)].all())              # (no addition, no difference)


def test_widths_and_shapes_reach_every_vec_lpr_pair():
    """The (kernel, VEC, LPR) triples of the bf16 instantiations the suite did not launch, by the dispatch rules restated in
    bf16_cases (``hop_structures.pick_lpr`` over 8-element packets)."""
    assert [hs.pick_lpr(d, 8) for d in (64, 65, 128, 129, 256, 257, 512, 520)] == [8, 16, 16, 32, 32, 64, 64, 64]
    seg = {w.id: bc.seg_geometry(w) for w in bc.SEG_WIDTHS}
    assert seg == {"d64": ("wave", 8, 8, 1), "d128": ("wave", 8, 16, 1), "d256": ("wave", 8, 32, 1), "d512": ("wave", 8, 64, 1),
                   "d520": ("wave", 8, 64, 2), "d20": ("wave", 1, 64, 1), "d70": ("wave", 1, 64, 2), "d64p68": ("wave", 1, 64, 1)}
    assert [bc.seg_geometry(w, 2) for w in bc.FLAT_WIDTHS] == [("flat", 8, lpr, 1) for lpr in (8, 16, 32, 64)]
    assert set(bc.BWD_WIDTHS) <= {w.d for w in bc.SEG_WIDTHS}
    pma = {s.id: bc.pma_geometry(s) for s in bc.PMA_SHAPES}
    assert pma == {"H3C4-v1": ("wave", 1, 64, 1), "H1C20-v1": ("wave", 1, 64, 1), "H2C36-v1": ("wave", 1, 64, 2),
                   "H1C64-v1": ("wave", 8, 8, 1), "H4C32-v1": ("wave", 8, 16, 1), "H8C32-v1": ("wave", 8, 32, 1),
                   "H8C64-v1": ("wave", 8, 64, 1), "H1C520-v1": ("wave", 8, 64, 2),
                   "H2C32-v2": ("flat", 8, 8, 1), "H4C32-v2": ("flat", 8, 16, 1), "H4C64-v2": ("flat", 8, 32, 1),
                   "H4C72-v2": ("flat", 8, 64, 1), "H8C64-v2": ("flat", 8, 64, 1)}
    stats = {bc.pma_stats_geometry(s)[:3] for s in bc.PMA_SHAPES}
    assert stats == {("wave", 1, 64), ("wave", 8, 64)} | {("flat", 8, lpr) for lpr in (8, 16, 32, 64)}
    assert len({s.id for s in bc.PMA_SHAPES}) == len(bc.PMA_SHAPES) == 13
    for s in bc.PMA_SHAPES:                                                        # a lane's packet never straddles a head
        assert bc.pma_geometry(s)[1] == 1 or s.C % 8 == 0


@pytest.mark.parametrize("flip", [False, True])
def test_pma_references_are_finite_and_consistent(flip):
    for s in (bc.PMA_SHAPES[0], bc.PMA_SHAPES[4], bc.PMA_SHAPES[11]):
        r = bc.pma_reference(s.H, s.C, flip)
        for k in ("out", "m", "l", "gV", "galpha"):
            assert bool(torch.isfinite(r[k]).all()), k
        assert _bf16_exact(r["V"]) and _bf16_exact(r["G"])
        assert bool((r["l"][r["empty"]] == 0).all()) and bool((r["l"][~r["empty"]] >= 1).all()) and bool(r["empty"].any())
        assert bool((r["out"][r["empty"]] == 0).all())
        # the statistics restated on the kernel's own inputs agree with the unrounded ones to the rounding of ``out``
        st = bc.pma_stats_reference(bc.bf16_round(r["out"]), r["G"], r["m"], r["l"], s.H)
        assert torch.equal(st[..., 0], r["stats"][..., 0])
        bound = 2.0 ** -8 * (r["out"].abs() * r["G"].abs()).view(r["n_t"], s.H, s.C).sum(-1)
        assert bool(((st[..., 1] - r["stats"][..., 1]).abs() <= bound).all())
        # gV is the transposed weighted sum of the cotangent: a second derivation of the oracle's gradient
        ei = bc.edges(flip)
        a = torch.nn.functional.leaky_relu(r["alpha"], bc.PMA_SLOPE)[ei[0]]
        p = torch.exp(a - r["stats"][ei[1], :, 0])
        gV = torch.zeros(r["n_s"], s.H, s.C, dtype=torch.float64).index_add(0, ei[0], p.unsqueeze(-1) * r["G"].view(-1, s.H, s.C)[ei[1]])
        torch.testing.assert_close(gV.view(r["n_s"], -1), r["gV"], rtol=1e-9, atol=1e-9)
