"""CPU: the cases tests/test_gpu_bf16_linear_steps.py runs, vouched for from the restated walk and from float64 alone -- the lists reach
all 40 instantiations of ``linear_bf16_kernel``, drive some wave through every step count from one to five, put the partial last chunk
into either register buffer by the loop and by the tail, and clamp a prefetch while its wave still has work; the restatement is tied
to three literals of csrc/fused_bf16.hip; the tables are representable; the rule accepts fp32 accumulation with one rounding on the
largest table and rejects the plausible wrong kernels on the tables themselves.  Everything is imported from
tests/bf16_linear_cases.py, the module the GPU file imports it from."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_linear_cases as lc  # noqa: E402

SOURCE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "allset_amd", "csrc", "fused_bf16.hip")
N_SHARP = lc.STEP_ROWS[4]                              # 2R + 16 * 1000 + 5: the row count the discrimination figures are measured at


@pytest.fixture(scope="module", autouse=True)
def _free_tables():
    yield
    lc.free_tables()


def _bf16_exact(t):
    return bool((t.float().bfloat16().double() == t).all())


def _share(bad):
    return float(bad.double().mean())


# ---- the restatement and the kernel ----------------------------------------------------------------------------------------------------
def test_the_restated_geometry_rests_on_three_literals_of_the_kernel():
    src = open(SOURCE).read()
    assert re.search(r"constexpr int kBfBlock = %d;" % lc.BLOCK, src)
    assert "constexpr int kBfWaves = kBfBlock / kWave;" in src and lc.WAVES == lc.BLOCK // lc.WAVE == 8
    assert "const int64_t n_chunks = (n + 15) / 16;" in src and "int64_t blocks = ((n + 15) / 16 + kBfWaves - 1) / kBfWaves;" in src
    assert lc.CHUNK_ROWS == 16
    assert "if (blocks > %d) blocks = %d;" % (lc.GRID_CAP, lc.GRID_CAP) in src
    assert lc.R == 32768 == lc.CHUNK_ROWS * lc.WAVES * lc.GRID_CAP
    assert [lc.grid(n) for n in (1, 128, 129, lc.R - 1, lc.R, lc.R + 1, 4 * lc.R + 1)] == [1, 1, 2, 256, 256, 256, 256]
    # the loop and the tail the walk follows
    assert "for (; chunk + stride < n_chunks; chunk += 2 * stride) {" in src and "if (chunk < n_chunks) process(a0, m0, chunk, DEPTH);" in src
    assert "prologue(a, m, chunk, chunk + stride);" in src and "request(a, x, ldx, chunk + ahead * stride);" in src


def test_row_counts_are_derived_from_the_sweep():
    R = lc.R
    assert lc.STEP_ROWS == (R - 1, R, R + 1, 2 * R + 1, 2 * R + 16 * 1000 + 5, 3 * R + 16 * 7 + 9, 4 * R + 1)
    assert max(lc.STEP_ROWS) == 4 * R + 1 == 131073
    assert lc.SMALL_ROWS == (1, 15, 16, 17, 129)


@pytest.mark.parametrize("n", lc.STEP_ROWS + lc.SMALL_ROWS)
def test_walk_covers_every_chunk_once_from_a_buffer_that_holds_it(n):
    """The replayed requests: every chunk is consumed exactly once, from a buffer whose latest (clamped) request was that chunk, with
    the mask buffer holding the same chunk."""
    waves = lc.walk(n)
    assert len(waves) == lc.WAVES * lc.grid(n)
    chunks = sorted(s.chunk for steps in waves for s in steps)
    assert chunks == list(range(lc.n_chunks(n)))
    for steps in waves:
        for i, s in enumerate(steps):
            assert s.held == s.chunk == s.mask_held, (n, s)
            assert s.buffer == ("a0", "a1")[i % 2]
            assert s.loaded_by == ("first" if i < 2 else steps[i - 2].where)


def test_steps_per_wave_and_the_last_chunk():
    R = lc.R
    want = {R - 1: ({1: 2048}, "a0", "tail", "first", 15), R: ({1: 2048}, "a0", "tail", "first", 16),
            R + 1: ({1: 2047, 2: 1}, "a1", "loop", "first", 1), 2 * R + 1: ({2: 2047, 3: 1}, "a0", "tail", "loop", 1),
            2 * R + 16 * 1000 + 5: ({2: 1047, 3: 1001}, "a0", "tail", "loop", 5),
            3 * R + 16 * 7 + 9: ({3: 2040, 4: 8}, "a1", "loop", "loop", 9), 4 * R + 1: ({4: 2047, 5: 1}, "a0", "tail", "loop", 1)}
    for n in lc.STEP_ROWS:
        s, rows = lc.last_chunk_step(n)
        assert (lc.steps_per_wave(n), s.buffer, s.where, s.loaded_by, rows) == want[n], n
    # 3R + 16 * 7 + 9: the last chunk is the second step of the SECOND loop trip of its wave
    steps = [st for st in lc.walk(3 * R + 16 * 7 + 9) if len(st) == 4][-1]
    assert [s.where for s in steps] == ["loop"] * 4 and steps[3].chunk == lc.n_chunks(3 * R + 16 * 7 + 9) - 1


def test_the_lists_reach_every_instantiation_and_every_step_count():
    for name, cases in (("step", lc.STEP_CASES), ("small", lc.SMALL_CASES)):
        assert {lc.instantiation(c.kind, c.KD, c.ND) for c in cases} == lc.all_instantiations(), name
    assert len(lc.all_instantiations()) == 40 and len(lc.KINDS) == 10
    for n in lc.ALL_KINDS_ROWS:                                                       # all 40 at each of the two row counts
        assert {lc.instantiation(c.kind, c.KD, c.ND) for c in lc.STEP_CASES if c.n == n} == lc.all_instantiations()
    for k in lc.KINDS:                                                                # all of STEP_ROWS on the 256 x 256 shape of every kind
        assert {c.n for c in lc.STEP_CASES if c.kind == k and (c.KD, c.ND) == (256, 256)} == set(lc.STEP_ROWS)
        assert {(c.n, c.KD, c.ND) for c in lc.SMALL_CASES if c.kind == k} == {(n, KD, ND) for n in lc.SMALL_ROWS for KD, ND in lc.SHAPES}
    assert len(lc.STEP_CASES) == 40 * 2 + 10 * 5 and len(lc.SMALL_CASES) == 200
    assert len({c.id for c in lc.STEP_CASES + lc.SMALL_CASES}) == 330
    counts = set()
    for n in {c.n for c in lc.STEP_CASES}:
        counts |= set(lc.steps_per_wave(n))
    assert counts == {1, 2, 3, 4, 5}
    # the run-time form (MASK 1) is one instantiation per shape whatever else it is given
    assert lc.select("bwd", 1, acc=True, aux_in=True) == lc.select("bwd", 1) == (True, 1, False, False)
    assert {c.n for c in lc.SENTINEL_CASES} == {2 * lc.R + 16 * 1000 + 5} and len(lc.SENTINEL_CASES) == 10
    assert lc.BITS_EQUAL_ROWS == (2 * lc.R + 1, 3 * lc.R + 16 * 7 + 9)


def test_the_partial_last_chunk_meets_both_buffers_the_loop_and_the_tail():
    """Over the step lists the partial last chunk is consumed from a0 by the tail (loaded by ``first_requests`` and, after a loop trip,
    by the loop's own two-steps-ahead request), and from a1 inside the loop (first and second trip).  It is never CONSUMED from a0
    inside the loop -- a0's loop step requires ``chunk + stride < n_chunks`` -- but it lands there as a clamped prefetch while the wave
    still has its a1 step to run (R + 1: wave 0 requests chunk 4096, gets the one-row chunk 2048, then consumes a1)."""
    seen = set()
    for n in lc.STEP_ROWS:
        s, rows = lc.last_chunk_step(n)
        if rows < lc.CHUNK_ROWS:
            seen.add((s.buffer, s.where, s.loaded_by))
    assert seen == {("a0", "tail", "first"), ("a0", "tail", "loop"), ("a1", "loop", "first"), ("a1", "loop", "loop")}
    for n in lc.STEP_ROWS + lc.SMALL_ROWS:
        last = lc.n_chunks(n) - 1
        assert not any(s.chunk == last and s.buffer == "a0" and s.where == "loop" for st in lc.walk(n) for s in st)
    steps = lc.walk(lc.R + 1)[0]
    assert [(s.buffer, s.where, s.clamped) for s in steps] == [("a0", "loop", True), ("a1", "loop", True)]
    assert lc.rows_here(lc.R + 1, lc.n_chunks(lc.R + 1) - 1) == 1


def test_some_prefetch_is_clamped_while_its_wave_still_has_a_step_to_run():
    for n in lc.STEP_ROWS[2:]:
        waves = lc.walk(n)
        assert any(s.clamped for st in waves for s in st[:-1]), n
    # and at the two row counts every instantiation runs at, so is a request that is NOT clamped: the buffers are really reused
    for n in lc.ALL_KINDS_ROWS:
        assert any(not s.clamped for st in lc.walk(n) for s in st)
        assert any(s.loaded_by == "loop" and s.buffer == "a1" for st in lc.walk(n) for s in st) == (n == lc.ALL_KINDS_ROWS[1])


def test_the_gap_this_closes():
    """At every row count the older direct comparisons use, no wave has a second step: the loop body, a1, the reuse of a0 and the
    mask's next request were never compared with anything."""
    for n in lc.OLD_ROWS:
        assert set(lc.steps_per_wave(n)) == {1}, n
        assert all(s.buffer == "a0" and s.where == "tail" for st in lc.walk(n) for s in st)
    assert max(lc.OLD_ROWS) < lc.R


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def test_tables_are_representable_and_rows_are_not_repeated():
    n = lc.STEP_ROWS[4]
    f, b = lc.tables(n, 256, 128, "fwd"), lc.tables(n, 128, 256, "bwd")
    for k in ("x", "W", "b", "aux_w", "aux_b"):
        assert _bf16_exact(f[k]), k
    for k in ("gy", "W", "ymask", "acc_in", "aux_w"):
        assert _bf16_exact(b[k]), k
    assert bool((b["galpha"].float().double() == b["galpha"]).all()) and not _bf16_exact(b["galpha"])
    assert tuple(b["W"].shape) == (128, 256) and tuple(f["W"].shape) == (128, 256) and tuple(b["acc_in"].shape) == (n, 256)
    # a row and the row one sweep later differ (a tiled table would make a step mix-up invisible)
    x = f["x"]
    assert not bool((x[:n - lc.R] == x[lc.R:]).all(1).any())
    ym = b["ymask"]
    assert bool((ym >= 0).all()) and 0.4 < _share(ym > 0) < 0.6
    for row in lc.ZERO_ROWS:
        z = ym[row] == 0
        neg = z & torch.signbit(ym[row])
        assert int(neg.sum()) >= 128 // 7 and int((z & ~neg).sum()) >= 128 // 7
        assert bool(torch.signbit(ym[row].to(torch.bfloat16))[neg].all())            # -0.0 survives the trip to bf16
        assert bool((b["gy"][row][z] != 0).all())                                    # and the gradient under every zero is visible
    assert lc.ZERO_ROWS == (1, lc.R + 1, 2 * lc.R + 1) and n > lc.ZERO_ROWS[2]
    assert lc.tables(n, 256, 128, "fwd") is f                                        # built once per key


def test_bit_order_round_trip():
    m = torch.from_numpy(np.random.default_rng(3).integers(0, 2, size=(37, 256)).astype(bool))
    for N in (128, 256):
        assert torch.equal(lc.decode_bits(lc.encode_bits(m[:, :N]), N), m[:, :N])
    one = torch.zeros(1, 256, dtype=torch.bool)
    one[0, 64 * 2 + 16 * 3 + 5] = True                                               # column 64 hb + 16 sq + j -> bit 16 hb + j of word sq
    word = lc.encode_bits(one).numpy().view("<u8")[0]
    assert int(word[3]) == 1 << (16 * 2 + 5)


# ---- the condition ---------------------------------------------------------------------------------------------------------------------
def test_unsure_pre_activations_stay_under_the_cap():
    """Every forward table a relu runs on (the mask-output kind of the lists; the backward bit masks come from the same tables): the
    share of elements whose float64 pre-activation is within UNSURE of zero stays under UNSURE_CAP (measured: at most 0.14 %)."""
    worst = 0.0
    keys = {(c.n, c.KD, c.ND) for c in lc.STEP_CASES + lc.SMALL_CASES if c.kind.id == "fwd-maskout"}
    for n, KD, ND in sorted(keys):
        share = lc.unsure_share(lc.tables(n, KD, ND, "fwd"))
        worst = max(worst, share)
        assert share <= lc.UNSURE_CAP, (n, KD, ND, share)
    print(f"unsure elements: at most {worst:.4%} of a table")


# ---- the rule is reachable -------------------------------------------------------------------------------------------------------------
def test_fp32_accumulation_with_one_rounding_is_inside_the_rule_on_the_largest_table():
    t = lc.tables(max(lc.STEP_ROWS), 256, 256, "fwd")
    ref = lc.fwd_reference(t, False)
    y32 = t["x"].float() @ t["W"].float().t() + t["b"].float()
    print(f"largest fp32 error {float((y32.double() - ref).abs().max()):.3e} on {ref.numel()} elements")
    assert float((y32.double() - ref).abs().max()) < 1e-5
    assert bool(lc.within_one_rounding(y32.bfloat16().double(), ref).all())
    assert bool(lc.within_one_rounding(torch.relu(y32).bfloat16().double(), lc.fwd_reference(t, True)).all())


# ---- the rule is sharp -----------------------------------------------------------------------------------------------------------------
# the shares measured on these tables; each assertion asks for half
FLOORS = dict(truncation=0.432, early_rounding=0.255, stride_row=0.998, mask_ge=0.993, neg_zero=0.989, no_acc=0.996, no_rank4=0.998)


def test_rule_rejects_the_wrong_forward_kernels():
    """On the 256 x 256 forward table at 2R + 16 * 1000 + 5 rows (20.9M elements; asserted: half the measured share): truncation at
    the store is rejected on 43.2 % of the elements, a rounding before the bias is added on 25.5 %, a row taken from the chunk one
    stride away on 99.8 %."""
    t = lc.tables(N_SHARP, 256, 256, "fwd")
    ref = lc.fwd_reference(t, False)
    assert bool(lc.within_one_rounding(lc.bf16_round(ref), ref).all())
    wrong = {"truncation": lc.truncate_bf16(ref),
             "early_rounding": lc.bf16_round(lc.bf16_round(t["P"]) + t["b"])}
    stride_rows = lc.CHUNK_ROWS * lc.WAVES * lc.grid(N_SHARP)
    src = (torch.arange(N_SHARP) + stride_rows) % N_SHARP                             # the row of the chunk one stride away
    wrong["stride_row"] = lc.bf16_round(ref)[src]
    for name, got in wrong.items():
        share = _share(~lc.within_one_rounding(got, ref))
        print(f"{name}: rejected on {share:.4f}")
        assert share >= 0.5 * FLOORS[name], name


def test_rule_rejects_the_wrong_backward_kernels():
    """On the 256 x 256 backward table at 2R + 16 * 1000 + 5 rows, the activation-masked form with both extra terms (asserted: half
    the measured share): ``>= 0`` for ``> 0`` is rejected on 99.4 % of the elements; a test that lets -0.0 through on 99.0 % of the
    elements of the three planted rows (and nowhere else); a missing ``acc_in`` on 99.6 %, a missing rank-4 term on 99.9 %."""
    t = lc.tables(N_SHARP, 256, 256, "bwd")
    full = lc.bwd_reference(t, "act", True, True)
    assert bool(lc.within_one_rounding(lc.bf16_round(full), full).all())
    gy, ym = t["gy"], t["ymask"]
    zero = torch.zeros((), dtype=lc.D64)
    ge = torch.where(ym >= 0, gy, zero) @ t["W"] + t["acc_in"] + t["galpha"] @ t["aux_w"]          # '>= 0': both zeros pass
    share = _share(~lc.within_one_rounding(lc.bf16_round(ge), full))
    print(f"mask_ge: rejected on {share:.4f}")
    assert share >= 0.5 * FLOORS["mask_ge"]
    # 'any magnitude or sign bit set': -0.0 passes, +0.0 does not -- wrong on the planted rows only
    rows = torch.tensor([r for r in lc.ZERO_ROWS if r < N_SHARP])
    nz = (ym[rows] > 0) | ((ym[rows] == 0) & torch.signbit(ym[rows]))
    bad = torch.where(nz, gy[rows], zero) @ t["W"] + t["acc_in"][rows] + t["galpha"][rows] @ t["aux_w"]
    share = _share(~lc.within_one_rounding(lc.bf16_round(bad), full[rows]))
    print(f"neg_zero: rejected on {share:.4f} of the planted rows")
    assert len(rows) == 3 and share >= 0.5 * FLOORS["neg_zero"]
    sel = lc.selection(t, "act")
    assert bool((sel[rows][ym[rows] == 0] == 0).all()) and not bool(lc.bits_equal(torch.where(nz, gy[rows], zero).bfloat16(), sel[rows].bfloat16()).all())
    for name, got in (("no_acc", lc.bwd_reference(t, "act", False, True)), ("no_rank4", lc.bwd_reference(t, "act", True, False))):
        share = _share(~lc.within_one_rounding(lc.bf16_round(got), full))
        print(f"{name}: rejected on {share:.4f}")
        assert share >= 0.5 * FLOORS[name], name
