"""GPU: the Linear kernels of the bf16 regime (csrc/fused_bf16.hip) past one step per wave.  The lists of tests/bf16_linear_cases.py
-- every one of the 40 instantiations at row counts where a wave runs two to five steps of the persistent loop, every step count on the
256 x 256 shape, and the small counts -- run through ``dense.linear_bf16_fwd`` / ``_fwd_mask`` / ``_bwd`` / ``_bwd_bits`` and are
compared with float64 on the same bf16 inputs under ``bf16_cases.within_one_rounding`` (half a bf16 ulp on top of the fp32 kernels' own
1e-4); the masked gradient must be bitwise the selection, the bit mask exactly ``y > 0`` of the stored output in the documented order,
the fp32 logits are held to ``close_fp32``.  tests/test_bf16_linear_cases_host.py vouches for the cases from the restated walk and
float64 alone.  A device result is never an expected value; the stored output of a real forward, read for its relu mask, is data.
Each test prints ``max |got - ref| / (ulp/2)`` before it asserts."""
import os
import sys
from collections import OrderedDict

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_linear_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
NAN = float("nan")
SENTINEL = -1232.0                                     # a bf16 value no table holds
SENTINEL_BYTE = 0xA5
PAD = 64                                               # columns a strided view's buffer is wider by; the view starts at column PAD / 2
SPARE_ROWS = 16                                        # one whole chunk of rows behind row n - 1

_DEV = OrderedDict()                                   # device copies of the cached tables and the layers' real forwards
DEV_ENTRIES = 4


@pytest.fixture(scope="module", autouse=True)
def _free_at_teardown():
    yield
    _DEV.clear()
    lc.free_tables()
    torch.cuda.empty_cache()


def _keep(key, make):
    if key in _DEV:
        _DEV.move_to_end(key)
        return _DEV[key]
    _DEV[key] = make()
    while len(_DEV) > DEV_ENTRIES:
        _DEV.popitem(last=False)
    return _DEV[key]


def _dev(t, device):
    """The table's tensors on the device in their storage types (bf16; the logits' gradient fp32)."""
    return _keep(t["key"], lambda: {k: v.to(torch.float32 if k == "galpha" else BF16).to(device) for k, v in t.items()
                                    if torch.is_tensor(v) and not k.startswith("P")})


def _layer_forward(n, I, O, device):
    """A real ``linear_bf16_fwd_mask`` of the layer (I -> O) on its forward table: the stored output, its bit mask and ``y > 0`` on
    the host -- what a backward behind that relu is given."""
    def make():
        from allset_amd import dense
        d = _dev(lc.tables(n, I, O, "fwd"), device)
        y, bits = dense.linear_bf16_fwd_mask(d["x"], d["W"], d["b"])
        mask = (y.float() > 0).cpu()
        assert 0.2 < float(mask.double().mean()) < 0.8
        return dict(y=y, bits=bits, mask=mask)
    return _keep(("layer", n, I, O), make)


def _selection_is_exact(ga, t, mask, what):
    want = lc.selection(t, mask).to(BF16)
    same = lc.bits_equal(ga, want)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements of the masked gradient are not the selection"


def _bits_are_the_mask(bits, y, N, what):
    assert bits.dtype == torch.uint8 and tuple(bits.shape) == (y.shape[0], N // 8), what
    assert torch.equal(lc.decode_bits(bits, N), (y.float() > 0).cpu()), f"{what}: bit = (y > 0) in the documented order"


def _run(c, device, variants=False):
    """One case through the wrappers against float64.  ``variants``: also the run-time switches the instantiation does not depend on
    (relu on and off, no bias, the masked gradient not asked for)."""
    from allset_amd import dense
    t, k = lc.case_tables(c), c.kind
    d = _dev(t, device)
    if k.id == "fwd":
        y, none = dense.linear_bf16_fwd(d["x"], d["W"], d["b"], False)
        assert none is None and y.dtype == BF16
        lc.assert_one_rounding(y, lc.fwd_reference(t, False), f"{c.id} y")
        if variants:
            y, _ = dense.linear_bf16_fwd(d["x"], d["W"], None, True)
            lc.assert_one_rounding(y, lc.fwd_reference(t, True, bias=False), f"{c.id} relu, no bias: y")
    elif k.id == "fwd-aux":
        y, aux = dense.linear_bf16_fwd(d["x"], d["W"], d["b"], False, d["aux_w"], d["aux_b"])
        lc.assert_one_rounding(y, lc.fwd_reference(t, False), f"{c.id} y")
        assert aux.dtype == torch.float32
        lc.close_fp32(aux, lc.aux_reference(t), f"{c.id} aux")
        if variants:
            y, aux = dense.linear_bf16_fwd(d["x"], d["W"], d["b"], True, d["aux_w"], None)
            lc.assert_one_rounding(y, lc.fwd_reference(t, True), f"{c.id} relu: y")
            lc.close_fp32(aux, lc.aux_reference(t) - t["aux_b"], f"{c.id} no aux_b: aux")
    elif k.id == "fwd-maskout":
        y, bits = dense.linear_bf16_fwd_mask(d["x"], d["W"], d["b"])
        lc.assert_one_rounding(y, lc.fwd_reference(t, True), f"{c.id} y")
        _bits_are_the_mask(bits, y, c.ND, c.id)
    elif k.mask_mode == 2:
        f = _layer_forward(c.n, c.ND, c.KD, device)
        gx = dense.linear_bf16_bwd_bits(d["gy"], d["W"], f["bits"], acc_in=d["acc_in"] if k.acc else None)
        lc.assert_one_rounding(gx, lc.bwd_reference(t, f["mask"], k.acc, False, tag="bits"), f"{c.id} gx")
    elif k.mask_mode == 1:
        gx, ga = dense.linear_bf16_bwd(d["gy"], d["W"], d["ymask"], want_ga=True, acc_in=d["acc_in"], galpha=d["galpha"], aux_w=d["aux_w"])
        _selection_is_exact(ga, t, "act", c.id)
        lc.assert_one_rounding(gx, lc.bwd_reference(t, "act", True, True), f"{c.id} with ga_out, acc_in and galpha: gx")
        if variants:
            gx, ga = dense.linear_bf16_bwd(d["gy"], d["W"], d["ymask"], want_ga=True)
            _selection_is_exact(ga, t, "act", c.id + " alone")
            lc.assert_one_rounding(gx, lc.bwd_reference(t, "act"), f"{c.id} alone: gx")
            gx, ga = dense.linear_bf16_bwd(d["gy"], d["W"], d["ymask"], want_ga=False, acc_in=d["acc_in"])
            assert ga is d["gy"]
            lc.assert_one_rounding(gx, lc.bwd_reference(t, "act", True, False), f"{c.id} no ga_out, acc_in: gx")
    else:
        gx, ga = dense.linear_bf16_bwd(d["gy"], d["W"], None, acc_in=d["acc_in"] if k.acc else None,
                                       galpha=d["galpha"] if k.aux_in else None, aux_w=d["aux_w"] if k.aux_in else None)
        assert ga is d["gy"]
        lc.assert_one_rounding(gx, lc.bwd_reference(t, None, k.acc, k.aux_in), f"{c.id} gx")


@pytest.mark.parametrize("c", lc.STEP_CASES, ids=lambda c: c.id)
def test_two_to_five_steps_per_wave_are_one_rounding_from_float64(c, device):
    _run(c, device)


@pytest.mark.parametrize("c", lc.SMALL_CASES, ids=lambda c: c.id)
def test_small_row_counts_are_one_rounding_from_float64(c, device):
    _run(c, device, variants=True)


# ---- strided views and what lies around the outputs --------------------------------------------------------------------------------------
def _wide_in(t, device):
    """A bf16 [n, w] device tensor as columns PAD / 2 .. of a buffer PAD columns wider whose other columns hold NaN."""
    n, w = t.shape
    buf = torch.full((n, w + PAD), NAN, dtype=BF16, device=device)
    buf[:, PAD // 2:PAD // 2 + w] = t
    v = buf[:, PAD // 2:PAD // 2 + w]
    assert v.stride(0) == w + PAD and v.data_ptr() % 16 == 0
    return v


class _Out:
    """An output of n rows and w columns inside a sentinel-filled buffer with SPARE_ROWS more rows and, where the entry takes a leading
    dimension, PAD more columns."""

    def __init__(self, n, w, dtype, device, strided):
        self.n, self.w = n, w
        self.c0 = PAD // 2 if strided else 0
        fill = SENTINEL_BYTE if dtype == torch.uint8 else SENTINEL
        self.fill = fill
        self.buf = torch.full((n + SPARE_ROWS, w + (PAD if strided else 0)), fill, dtype=dtype, device=device)
        self.view = self.buf[:n, self.c0:self.c0 + w]
        assert self.view.data_ptr() % 16 == 0

    def check(self, want, what):
        assert torch.equal(self.view, want), f"{what}: the strided result differs from the dense one"
        rest = self.buf.clone()
        rest[:self.n, self.c0:self.c0 + self.w] = self.fill
        assert bool((rest == self.fill).all()), f"{what}: {int((rest != self.fill).sum())} elements outside the output were written"


@pytest.mark.parametrize("c", lc.SENTINEL_CASES, ids=lambda c: c.id)
def test_strided_views_give_the_same_bits_and_nothing_else_is_written(c, device):
    """The C entries called the way dense.py calls them, on column views of wider buffers (inputs between NaN columns, outputs between
    sentinel columns and in front of sixteen sentinel rows): bitwise the dense wrappers' results -- which the step list above holds to
    float64 -- and every sentinel intact, in y, gx, ga_out, aux_out and the bit mask."""
    from allset_amd import dense, _lib
    from allset_amd._lib import check, ptr, stream_of
    from allset_amd.ops import _ld
    lib = _lib.load()
    t, k, n = lc.case_tables(c), c.kind, c.n
    d = _dev(t, device)
    st = stream_of(device)
    if k.direction == "fwd":
        K, N = c.KD, c.ND
        x = _wide_in(d["x"], device)
        y = _Out(n, N, BF16, device, True)
        if k.id == "fwd-maskout":
            y0, bits0 = dense.linear_bf16_fwd_mask(d["x"], d["W"], d["b"])
            bits = _Out(n, N // 8, torch.uint8, device, False)
            check(lib.allset_linear_bf16_fwd_mask(ptr(x), _ld(x), ptr(d["W"]), ptr(d["b"]), ptr(y.view), _ld(y.view), ptr(bits.buf), n, K, N, st),
                  "allset_linear_bf16_fwd_mask")
            bits.check(bits0, c.id + " bits")
        else:
            with_aux = k.id == "fwd-aux"
            y0, aux0 = dense.linear_bf16_fwd(d["x"], d["W"], d["b"], False, d["aux_w"] if with_aux else None, d["aux_b"] if with_aux else None)
            aux = _Out(n, 4, torch.float32, device, False) if with_aux else None
            check(lib.allset_linear_bf16_fwd(ptr(x), _ld(x), ptr(d["W"]), ptr(d["b"]), 0, ptr(d["aux_w"]) if with_aux else 0,
                                             ptr(d["aux_b"]) if with_aux else 0, ptr(aux.buf) if with_aux else 0, ptr(y.view), _ld(y.view),
                                             n, K, N, st), "allset_linear_bf16_fwd")
            if with_aux:
                aux.check(aux0, c.id + " aux")
        y.check(y0, c.id + " y")
        return
    O, I = c.KD, c.ND
    gy = _wide_in(d["gy"], device)
    acc = _wide_in(d["acc_in"], device)
    gx = _Out(n, I, BF16, device, True)
    if k.mask_mode == 2:
        f = _layer_forward(n, I, O, device)
        gx0 = dense.linear_bf16_bwd_bits(d["gy"], d["W"], f["bits"], acc_in=d["acc_in"] if k.acc else None)
        check(lib.allset_linear_bf16_bwd_bits(ptr(gy), _ld(gy), ptr(f["bits"]), ptr(d["W"]), ptr(acc) if k.acc else 0, _ld(acc) if k.acc else 0,
                                              ptr(gx.view), _ld(gx.view), n, O, I, st), "allset_linear_bf16_bwd_bits")
    elif k.mask_mode == 1:
        ym = _wide_in(d["ymask"], device)
        ga = _Out(n, O, BF16, device, True)
        gx0, ga0 = dense.linear_bf16_bwd(d["gy"], d["W"], d["ymask"], want_ga=True, acc_in=d["acc_in"], galpha=d["galpha"], aux_w=d["aux_w"])
        check(lib.allset_linear_bf16_bwd(ptr(gy), _ld(gy), ptr(ym), _ld(ym), ptr(ga.view), _ld(ga.view), ptr(d["W"]), ptr(d["galpha"]),
                                         ptr(d["aux_w"]), ptr(acc), _ld(acc), ptr(gx.view), _ld(gx.view), n, O, I, st), "allset_linear_bf16_bwd")
        ga.check(ga0, c.id + " ga_out")
    else:
        gx0, _ = dense.linear_bf16_bwd(d["gy"], d["W"], None, acc_in=d["acc_in"] if k.acc else None,
                                       galpha=d["galpha"] if k.aux_in else None, aux_w=d["aux_w"] if k.aux_in else None)
        check(lib.allset_linear_bf16_bwd(ptr(gy), _ld(gy), 0, 0, 0, 0, ptr(d["W"]), ptr(d["galpha"]) if k.aux_in else 0,
                                         ptr(d["aux_w"]) if k.aux_in else 0, ptr(acc) if k.acc else 0, _ld(acc) if k.acc else 0,
                                         ptr(gx.view), _ld(gx.view), n, O, I, st), "allset_linear_bf16_bwd")
    gx.check(gx0, c.id + " gx")


# ---- the two encodings of one mask -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", lc.BITS_EQUAL_ROWS)
@pytest.mark.parametrize("acc", [False, True], ids=["", "acc"])
def test_backward_from_bits_is_bitwise_the_activation_masked_form(n, acc, device):
    """Same arithmetic, only the mask's encoding (and with it the instantiation: one mask buffer of two bytes per element against
    one of two bytes per sixteen) differs: bit-identical gx where the last chunk is met by the tail and inside the second loop trip."""
    from allset_amd import dense
    d = _dev(lc.tables(n, 256, 256, "bwd"), device)
    f = _layer_forward(n, 256, 256, device)
    a = d["acc_in"] if acc else None
    gx0, _ = dense.linear_bf16_bwd(d["gy"], d["W"], f["y"], want_ga=True, acc_in=a)
    gx = dense.linear_bf16_bwd_bits(d["gy"], d["W"], f["bits"], acc_in=a)
    assert torch.equal(gx, gx0)


# ---- PMA's projection: the auxiliary columns forward, the rank-4 term backward, the four rows of the weight gradient --------------------
@pytest.mark.parametrize("H", lc.PMA_HEADS)
def test_pma_projection_node_at_three_steps_per_wave(H, device):
    """``dense.pma_project_bf16`` 256 -> 256 with H = 4 and H = 2 logits (the node pads the auxiliary rows with zeros): values, logits,
    gx under the Linear's rules; the weight gradients against float64 under the rule tests/bf16_dense_cases.py holds them to (one
    rounding; the logits' gradient is rounded to bf16 where it enters the weight-gradient pass)."""
    from allset_amd import dense
    n = lc.PMA_ROWS
    t, tb = lc.tables(n, 256, 256, "fwd"), lc.tables(n, 256, 256, "bwd")
    d, db = _dev(t, device), _dev(tb, device)
    leaves = [d[k].clone().requires_grad_(True) for k in ("x", "W", "b")] + [d["aux_w"][:H].clone().requires_grad_(True),
                                                                              d["aux_b"][:H].clone().requires_grad_(True)]
    xv, alpha = dense.pma_project_bf16(*leaves)
    assert xv.dtype == BF16 and alpha.dtype == torch.float32 and tuple(alpha.shape) == (n, H)
    what = f"pma_project H{H}"
    lc.assert_one_rounding(xv, lc.fwd_reference(t, False), what + " x_v")
    lc.close_fp32(alpha, lc.aux_reference(t)[:, :H], what + " alpha")
    g_alpha = db["galpha"][:, :H].contiguous()
    torch.autograd.backward([xv, alpha], [db["gy"], g_alpha])
    gv, g4, w_a = tb["gy"], tb["galpha"][:, :H], t["aux_w"][:H]
    lc.assert_one_rounding(leaves[0].grad, gv @ t["W"] + g4 @ w_a, what + " gx")
    gwv, gbv, gwa, gba = lc.wgrad_reference(gv, t["x"], None, g4)
    for got, ref, name in zip(leaves[1:], (gwv, gbv, gwa, gba), ("gW_v", "gb_v", "gW_a", "gb_a")):
        assert got.grad.dtype == BF16
        lc.assert_one_rounding(got.grad, ref, f"{what} {name}")
