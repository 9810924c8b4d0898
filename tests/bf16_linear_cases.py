"""The Linear of the bf16 regime (csrc/fused_bf16.hip, ``linear_bf16_kernel<KD, ND, TRANS_W, MASK, AUX, EXTRA>``): the persistent
walk restated, the row counts that drive a wave through one to five steps, the lists that reach all 40 instantiations, the input
tables, their float64 references and the acceptance rule.  Imports on the CPU; shared by tests/test_bf16_linear_cases_host.py (which
vouches for every case from float64 and the restated walk alone) and tests/test_gpu_bf16_linear_steps.py (which runs the same lists
through the HIP kernels), so the two cannot drift.

The kernel is persistent: ``grid(n)`` workgroups of 8 waves, capped at 256; a wave owns the 16-row chunk ``8 block + wave`` and then
every ``stride = 8 grid`` chunks after it.  Two register buffers ``a0`` / ``a1`` alternate, each requested two steps ahead; ONE mask
buffer ``m0`` is requested one step ahead; every request past the end is clamped to the last chunk; the steps run as a two-step loop
plus a peeled tail.  A wave takes a second step only above ``R = 16 * 8 * 256`` rows: everything here is derived from ``R``.

The rounding rule, the exact-bits comparison and the fp32 rule are those of tests/bf16_cases.py, imported and not restated: the kernel
accumulates in fp32 and rounds ONCE, at the store.  All tables are float64 holding bf16- (rows, parameters, cotangents, the other
gradient branch) or fp32- (the logits' gradient) representable numbers; every reference is float64 on those stored values."""
from __future__ import annotations

import os
import sys
from collections import OrderedDict, namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_structures as hs  # noqa: E402
from bf16_cases import (bf16_round, ulp_bf16, within_one_rounding, assert_one_rounding, bits_equal, close_fp32,  # noqa: E402,F401
                        half_ulps, ROUNDING_GOVERNS)
from bf16_dense_cases import UNSURE, UNSURE_CAP, truncate_bf16, wgrad_reference  # noqa: E402,F401

D64 = torch.float64

# ---- geometry (csrc/fused_bf16.hip restated; the host file reads the three literals out of the source) ---------------------------------
CHUNK_ROWS = 16                                        # rows of one step of one wave (one MFMA tile of rows)
BLOCK = 512                                            # kBfBlock
WAVE = 64                                              # common.h kWave
WAVES = BLOCK // WAVE                                  # kBfWaves
GRID_CAP = 256                                         # bf16_grid: one persistent workgroup per CU
WIDTHS = (128, 256)
SHAPES = [(KD, ND) for KD in WIDTHS for ND in WIDTHS]  # (reduction width, output width)


def n_chunks(n):
    return -(-n // CHUNK_ROWS)


def grid(n):
    """``bf16_grid``."""
    return max(1, min(GRID_CAP, -(-n_chunks(n) // WAVES)))


R = CHUNK_ROWS * WAVES * GRID_CAP                      # rows of one sweep of the full grid: 32768


def rows_here(n, chunk):
    return min(CHUNK_ROWS, n - chunk * CHUNK_ROWS)


Step = namedtuple("Step", "buffer chunk where held loaded_by mask_held clamped")
Step.__doc__ = """One ``process`` call of one wave.  ``buffer`` 'a0' / 'a1' and ``chunk``: what the kernel passes; ``where`` 'loop' /
'tail': the statement that ran it; ``held``: the chunk whose rows the buffer holds at that moment (after the clamp) and ``loaded_by``
the request that put them there ('first' = ``first_requests``, else the ``where`` of the step that requested them); ``mask_held``: the
chunk the one mask buffer holds; ``clamped``: this step's own request (``chunk + 2 stride``) is past the end."""


def walk(n):
    """For every wave of the launch (``8 grid(n)`` of them, in chunk order of their first step) its list of steps, statement by
    statement as the kernel runs them: ``first_requests``, the two-step loop, the peeled tail, and inside ``process`` the mask request
    for ``chunk + stride`` and the row request for ``chunk + 2 stride`` into the buffer just consumed."""
    nc = n_chunks(n)
    stride = WAVES * grid(n)
    clamp = lambda c: min(c, nc - 1)
    waves = []
    for first in range(stride):
        hold = {"a0": (clamp(first), "first"), "a1": (clamp(first + stride), "first")}
        mask = [clamp(first)]
        steps = []

        def process(buf, chunk, where):
            held, by = hold[buf]
            steps.append(Step(buf, chunk, where, held, by, mask[0], chunk + 2 * stride >= nc))
            mask[0] = clamp(chunk + stride)
            hold[buf] = (clamp(chunk + 2 * stride), where)
        chunk = first
        while chunk + stride < nc:
            process("a0", chunk, "loop")
            process("a1", chunk + stride, "loop")
            chunk += 2 * stride
        if chunk < nc:
            process("a0", chunk, "tail")
        waves.append(steps)
    return waves


def steps_per_wave(n):
    """{step count: waves} over the waves that have a chunk at all."""
    out = {}
    for s in walk(n):
        if s:
            out[len(s)] = out.get(len(s), 0) + 1
    return out


def last_chunk_step(n):
    """The step that consumes the last chunk, and the rows that chunk has."""
    last = n_chunks(n) - 1
    hits = [s for steps in walk(n) for s in steps if s.chunk == last]
    assert len(hits) == 1
    return hits[0], rows_here(n, last)


# ---- row counts: all derived from R --------------------------------------------------------------------------------------------------
STEP_ROWS = (R - 1, R, R + 1, 2 * R + 1, 2 * R + CHUNK_ROWS * 1000 + 5, 3 * R + CHUNK_ROWS * 7 + 9, 4 * R + 1)
ALL_KINDS_ROWS = (STEP_ROWS[4], STEP_ROWS[5])          # every instantiation runs at these two
SMALL_ROWS = (1, 15, 16, 17, 129)
OLD_ROWS = (1, 15, 16, 17, 129, 1000, 4099, 3000, 5000)   # what tests/test_gpu_bf16_linear.py compares at: one step per wave
ZERO_ROWS = (1, R + 1, 2 * R + 1)                      # rows of the first, second and third sweep that carry -0.0 and +0.0 in the mask

# ---- instantiations (launch_bf16 restated) ---------------------------------------------------------------------------------------------
Kind = namedtuple("Kind", "id direction mask_mode aux_out mask_out acc aux_in")
FWD_KINDS = [Kind("fwd", "fwd", 0, False, False, False, False),
             Kind("fwd-aux", "fwd", 0, True, False, False, False),
             Kind("fwd-maskout", "fwd", 0, False, True, False, False)]
BWD_KINDS = [Kind("bwd-bits", "bwd", 2, False, False, False, False),
             Kind("bwd-bits-acc", "bwd", 2, False, False, True, False),
             Kind("bwd-act", "bwd", 1, False, False, False, False),      # the run-time form: ga_out, acc_in and galpha are arguments
             Kind("bwd", "bwd", 0, False, False, False, False),
             Kind("bwd-acc", "bwd", 0, False, False, True, False),
             Kind("bwd-aux", "bwd", 0, False, False, False, True),
             Kind("bwd-acc-aux", "bwd", 0, False, False, True, True)]
KINDS = FWD_KINDS + BWD_KINDS


def select(direction, mask_mode=0, aux_out=False, mask_out=False, acc=False, aux_in=False):
    """``(TRANS_W, MASK, AUX, EXTRA)`` that ``launch_bf16`` picks for these arguments."""
    if direction == "fwd":
        if aux_out:
            return (False, 0, True, False)
        return (False, 0, False, bool(mask_out))
    if mask_mode == 2:
        return (True, 2, False, bool(acc))
    if mask_mode == 1:
        return (True, 1, False, False)
    return (True, 0, bool(aux_in), bool(acc))


def instantiation(kind, KD, ND):
    return (KD, ND) + select(kind.direction, kind.mask_mode, kind.aux_out, kind.mask_out, kind.acc, kind.aux_in)


def all_instantiations():
    """Every ``ALLSET_BF16_GO`` line of ``launch_bf16`` at every shape: 3 forward and 7 backward-data forms times 4 shapes."""
    fwd = [(False, 0, True, False), (False, 0, False, True), (False, 0, False, False)]
    bwd = [(True, 2, False, True), (True, 2, False, False), (True, 1, False, False), (True, 0, True, True), (True, 0, False, True),
           (True, 0, True, False), (True, 0, False, False)]
    return {(KD, ND) + t for KD, ND in SHAPES for t in fwd + bwd}


# ---- case lists ------------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id kind n KD ND")


def _case(kind, n, KD, ND):
    return Case(f"{kind.id}-n{n}-{KD}x{ND}", kind, n, KD, ND)


def layer_of(c):
    """(in, out) features of the layer the case belongs to: backward-data reduces over the layer's outputs."""
    return (c.KD, c.ND) if c.kind.direction == "fwd" else (c.ND, c.KD)


def _ordered(cases):
    """Unique, and grouped so that the cases of one table follow each other and the forward of a layer precedes its backward (whose
    bit mask it supplies): the table cache below then builds every table once."""
    seen = {}
    for c in cases:
        seen.setdefault(c.id, c)
    return sorted(seen.values(), key=lambda c: (c.n,) + layer_of(c) + (c.kind.direction != "fwd", KINDS.index(c.kind)))


STEP_CASES = _ordered([_case(k, n, KD, ND) for k in KINDS for KD, ND in SHAPES for n in ALL_KINDS_ROWS] +
                      [_case(k, n, 256, 256) for k in KINDS for n in STEP_ROWS])
SMALL_CASES = _ordered([_case(k, n, KD, ND) for k in KINDS for KD, ND in SHAPES for n in SMALL_ROWS])
SENTINEL_CASES = [_case(k, STEP_ROWS[4], 256, 256) for k in KINDS]
BITS_EQUAL_ROWS = (STEP_ROWS[3], STEP_ROWS[5])
PMA_ROWS, PMA_HEADS = STEP_ROWS[4], (4, 2)


# ---- tables ----------------------------------------------------------------------------------------------------------------------------
def _rng(*parts):
    return np.random.default_rng(hs.hash_id("linear-" + "-".join(str(p) for p in parts)))


def _randn(r, *shape, scale=1.0):
    """``randn`` (drawn in fp32: a rounding on the way to bf16 that changes nothing the tests rely on) rounded to bf16 ONCE.  Never
    a tiled smaller block: identical rows would hide a step mix-up."""
    return (torch.from_numpy(r.standard_normal(shape, dtype=np.float32)) * scale).bfloat16().double()


_CACHE = OrderedDict()
CACHE_ENTRIES = 3


def free_tables():
    _CACHE.clear()


def tables(n, KD, ND, direction):
    """The tables of ``(n, KD, ND, direction)``, built once per key (the largest takes over a second, its float64 product half of
    one) and kept for the few keys in use; the float64 base products are added to the same dict by the reference functions.
      fwd: x [n, KD], W [ND, KD] = randn / sqrt(KD), b [ND], aux_w [4, KD] = randn / sqrt(KD), aux_b [4];
      bwd: gy [n, KD], W [KD, ND] = randn / sqrt(KD) (the layer's [out, in] weight), ymask [n, KD] = a bf16 relu output with -0.0 and
           +0.0 planted on ``ZERO_ROWS``, acc_in [n, ND], galpha [n, 4] (fp32), aux_w [4, ND]."""
    key = (n, KD, ND, direction)
    if key in _CACHE:
        _CACHE.move_to_end(key)
        return _CACHE[key]
    r = _rng(*key)
    s = KD ** -0.5
    if direction == "fwd":
        t = dict(x=_randn(r, n, KD), W=_randn(r, ND, KD, scale=s), b=_randn(r, ND), aux_w=_randn(r, 4, KD, scale=s), aux_b=_randn(r, 4))
    else:
        ymask = torch.relu(_randn(r, n, KD))
        for row in ZERO_ROWS:
            if row < n:
                ymask[row, 0::7] = -0.0
                ymask[row, 1::7] = 0.0
        t = dict(gy=_randn(r, n, KD), W=_randn(r, KD, ND, scale=s), ymask=ymask, acc_in=_randn(r, n, ND),
                 galpha=torch.from_numpy(r.standard_normal((n, 4), dtype=np.float32)).double(), aux_w=_randn(r, 4, ND))
    t["key"] = key
    _CACHE[key] = t
    while len(_CACHE) > CACHE_ENTRIES:
        _CACHE.popitem(last=False)
    return t


def case_tables(c):
    return tables(c.n, c.KD, c.ND, c.kind.direction)


# ---- float64 references ----------------------------------------------------------------------------------------------------------------
def fwd_pre(t, bias=True):
    """``x W^T + b`` before the activation (the base product is kept on the table)."""
    if "P" not in t:
        t["P"] = t["x"] @ t["W"].t()
    return t["P"] + t["b"] if bias else t["P"]


def fwd_reference(t, relu, bias=True):
    pre = fwd_pre(t, bias)
    return torch.relu(pre) if relu else pre


def aux_reference(t):
    return t["x"] @ t["aux_w"].t() + t["aux_b"]


def selection(t, mask):
    """``ga``: gy where the mask is set, +0 elsewhere.  ``mask``: None, 'act' (``ymask > 0``: both zeros are not positive) or a bool
    tensor (the stored output of a real forward, ``y > 0``)."""
    if mask is None:
        return t["gy"]
    m = t["ymask"] > 0 if isinstance(mask, str) else mask
    return torch.where(m, t["gy"], torch.zeros((), dtype=D64))


def bwd_reference(t, mask=None, acc=False, aux=False, tag=None):
    """``gx = (gy where mask) W [+ acc_in] [+ galpha aux_w]``.  The product is kept on the table under ``tag`` (None: unmasked, 'act',
    or the caller's name for a bool mask -- one name per table and mask)."""
    name = "P" if mask is None else "P-" + (mask if isinstance(mask, str) else tag)
    if name not in t:
        t[name] = selection(t, mask) @ t["W"]
    ref = t[name]
    if acc:
        ref = ref + t["acc_in"]
    if aux:
        ref = ref + t["galpha"] @ t["aux_w"]
    return ref


def unsure_share(t):
    """Share of the elements whose float64 pre-activation is within ``UNSURE`` of zero: where a relu zero is no mask evidence."""
    return float((fwd_pre(t).abs() <= UNSURE).double().mean())


# ---- the bit mask ----------------------------------------------------------------------------------------------------------------------
def decode_bits(bits, N):
    """uint8 [n, N / 8] in the kernels' private order -> bool [n, N]: a row is four words of N / 32 bytes (little-endian); bit
    16 hb + j of word sq is column 64 hb + 16 sq + j (include/allset_hip_ext.h)."""
    b = bits.cpu().numpy()
    n = b.shape[0]
    ws = N // 32
    flat = np.unpackbits(b, axis=1, bitorder="little").reshape(n, 4, ws * 8)          # [row, sq, bit]
    out = np.zeros((n, N), dtype=bool)
    for sq in range(4):
        for hb in range(N // 64):
            out[:, 64 * hb + 16 * sq:64 * hb + 16 * sq + 16] = flat[:, sq, 16 * hb:16 * hb + 16].astype(bool)
    return torch.from_numpy(out)


def encode_bits(mask):
    """The inverse, for the host file: bool [n, N] -> uint8 [n, N / 8]."""
    m = mask.numpy()
    n, N = m.shape
    flat = np.zeros((n, 4, N // 4), dtype=np.uint8)
    for sq in range(4):
        for hb in range(N // 64):
            flat[:, sq, 16 * hb:16 * hb + 16] = m[:, 64 * hb + 16 * sq:64 * hb + 16 * sq + 16]
    return torch.from_numpy(np.packbits(flat.reshape(n, N), axis=1, bitorder="little"))
