"""GPU: the bf16-regime Linear kernels (csrc/fused_bf16.hip) against float64 of the same arithmetic on the same bf16 inputs.  The
kernels accumulate in fp32 and round ONCE to bf16, so the bound is ``bf16_cases.within_one_rounding``: half a bf16 ulp on top of the
fp32 kernels' own 1e-4.  Every row count here is one step per wave of the persistent kernel; tests/test_gpu_bf16_linear_steps.py
runs the same kernels through two to five."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bf16_linear_cases import assert_one_rounding, decode_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(256, 256), (128, 128), (256, 128), (128, 256)]
ROWS = [1, 15, 16, 17, 129, 1000, 4099]


def d64(t):
    return t.detach().double().cpu()


def bf(t, device):
    return t.to(torch.bfloat16).to(device)


@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("relu", [False, True])
def test_forward_matches_fp32_reference(K, N, n, relu, device):
    from allset_amd import dense
    g = torch.Generator().manual_seed(n * 7 + K + 3 * N + int(relu))
    x, W, b = bf(torch.randn(n, K, generator=g), device), bf(torch.randn(N, K, generator=g) / K ** 0.5, device), bf(torch.randn(N, generator=g), device)
    aw, ab = bf(torch.randn(4, K, generator=g) / K ** 0.5, device), bf(torch.randn(4, generator=g), device)
    y, aux = dense.linear_bf16_fwd(x, W, b, relu, aw, ab)
    ref = d64(x) @ d64(W).t() + d64(b)
    assert_one_rounding(y, F.relu(ref) if relu else ref, "y")
    torch.testing.assert_close(aux.cpu().double(), d64(x) @ d64(aw).t() + d64(ab), rtol=1e-5, atol=1e-5)
    y2, none = dense.linear_bf16_fwd(x, W, None, relu)
    assert none is None
    ref2 = d64(x) @ d64(W).t()
    assert_one_rounding(y2, F.relu(ref2) if relu else ref2, "y without bias")


@pytest.mark.parametrize("O,I", SHAPES)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("mask,acc,aux", [(False, False, False), (True, False, False), (True, True, False), (False, False, True),
                                          (False, True, True), (True, True, True)])
def test_backward_data_matches_fp32_reference(O, I, n, mask, acc, aux, device):
    from allset_amd import dense
    g = torch.Generator().manual_seed(n * 11 + O + 5 * I + 4 * mask + 2 * acc + aux)
    gy, W = bf(torch.randn(n, O, generator=g), device), bf(torch.randn(O, I, generator=g) / O ** 0.5, device)
    y = bf(F.relu(torch.randn(n, O, generator=g)), device) if mask else None
    if mask and n > 1:
        y[1, 3] = -0.0                                     # a negative zero is not "> 0"
    a = bf(torch.randn(n, I, generator=g), device) if acc else None
    ga4 = torch.randn(n, 4, generator=g).to(device) if aux else None
    aw = bf(torch.randn(4, I, generator=g), device) if aux else None
    gx, ga = dense.linear_bf16_bwd(gy, W, y, want_ga=mask, acc_in=a, galpha=ga4, aux_w=aw)
    ga_ref = torch.where(y.float() > 0, gy.float(), torch.zeros((), device=device)) if mask else gy.float()
    assert torch.equal(ga.float(), ga_ref), "the masked gradient is a selection, exact"
    ref = d64(ga_ref) @ d64(W)
    if acc:
        ref = ref + d64(a)
    if aux:
        ref = ref + d64(ga4) @ d64(aw)
    assert_one_rounding(gx, ref, "gx")


def test_rows_with_a_leading_dimension(device):
    """Row-strided views (columns of a wider buffer) are taken without a copy."""
    from allset_amd import dense
    g = torch.Generator().manual_seed(5)
    big = bf(torch.randn(700, 512, generator=g), device)
    x = big[:, 256:]
    W, b = bf(torch.randn(256, 256, generator=g) / 16, device), bf(torch.randn(256, generator=g), device)
    y, _ = dense.linear_bf16_fwd(x, W, b, True)
    assert_one_rounding(y, F.relu(d64(x) @ d64(W).t() + d64(b)), "y")
    gx, _ = dense.linear_bf16_bwd(x, W, big[:, :256], want_ga=False)
    assert_one_rounding(gx, torch.where(d64(big[:, :256]) > 0, d64(x), torch.zeros((), dtype=torch.float64)) @ d64(W), "gx")


@pytest.mark.parametrize("relu", [False, True])
def test_autograd_node_against_torch_fp32(relu, device):
    from allset_amd import dense
    g = torch.Generator().manual_seed(17 + relu)
    n, K, N = 3000, 256, 256
    x, W, b = bf(torch.randn(n, K, generator=g), device), bf(torch.randn(N, K, generator=g) / 16, device), bf(torch.randn(N, generator=g), device)
    G = bf(torch.randn(n, N, generator=g), device)
    xs, Ws, bs = (t.clone().requires_grad_(True) for t in (x, W, b))
    y = dense.linear_bf16(xs, Ws, bs, relu)
    y.backward(G)
    yr = d64(x) @ d64(W).t() + d64(b)
    yr = F.relu(yr) if relu else yr
    # the reference backward uses the mask of the stored bf16 output, as the kernels (and torch's bf16 relu) do
    gr = torch.where(d64(y) > 0, d64(G), torch.zeros((), dtype=torch.float64)) if relu else d64(G)
    assert_one_rounding(y, yr, "y")
    assert_one_rounding(xs.grad, gr @ d64(W), "gx")
    assert_one_rounding(Ws.grad, gr.t() @ d64(x), "gW")
    assert_one_rounding(bs.grad, gr.sum(0), "gb")


def test_unsupported_widths_fail_loudly(device):
    from allset_amd import dense, _lib
    x = torch.zeros(8, 64, dtype=torch.bfloat16, device=device)
    W = torch.zeros(64, 64, dtype=torch.bfloat16, device=device)
    assert not dense.linear_bf16_supported(x, W)
    with pytest.raises(_lib.AllSetHipError):
        dense.linear_bf16_fwd(x, W, None)


# ---- round 6: the relu mask as one bit per element (allset_linear_bf16_fwd_mask / _bwd_bits / allset_wgrad_bf16_ex2) ----------
@pytest.mark.parametrize("K,N", SHAPES)
@pytest.mark.parametrize("n", ROWS)
def test_forward_with_bit_mask_is_the_plain_forward_plus_its_mask(K, N, n, device):
    from allset_amd import dense
    g = torch.Generator().manual_seed(n * 13 + K + 3 * N)
    x, W, b = bf(torch.randn(n, K, generator=g), device), bf(torch.randn(N, K, generator=g) / K ** 0.5, device), bf(torch.randn(N, generator=g), device)
    y0, _ = dense.linear_bf16_fwd(x, W, b, True)
    y, bits = dense.linear_bf16_fwd_mask(x, W, b)
    assert torch.equal(y, y0), "the mask output must not change y"
    assert bits.shape == (n, N // 8) and bits.dtype == torch.uint8
    assert torch.equal(decode_bits(bits, N), (y.float() > 0).cpu()), "bit = (y > 0) in the documented order"


@pytest.mark.parametrize("O,I", SHAPES)
@pytest.mark.parametrize("n", ROWS)
@pytest.mark.parametrize("acc", [False, True])
def test_backward_data_from_bits_equals_the_activation_masked_form(O, I, n, acc, device):
    """Same kernel, same arithmetic, only the mask's encoding differs: bit-identical gx."""
    from allset_amd import dense
    g = torch.Generator().manual_seed(n * 17 + O + 5 * I + acc)
    u, Wf, bfw = bf(torch.randn(n, I, generator=g), device), bf(torch.randn(O, I, generator=g) / I ** 0.5, device), bf(torch.randn(O, generator=g), device)
    y, bits = dense.linear_bf16_fwd_mask(u, Wf, bfw)                      # a real forward: the mask of y = relu(u Wf^T + b)
    gy = bf(torch.randn(n, O, generator=g), device)
    a = bf(torch.randn(n, I, generator=g), device) if acc else None
    gx0, ga0 = dense.linear_bf16_bwd(gy, Wf, y, want_ga=True, acc_in=a)
    gx = dense.linear_bf16_bwd_bits(gy, Wf, bits, acc_in=a)
    assert torch.equal(gx, gx0)
    # and the weight gradient with the mask applied in its staging equals the one computed from the stored masked gradient
    gw0, gb0 = dense.wgrad(ga0, u, want_bias=True)
    gw, gb = dense.wgrad_bf16_ex2(gy, u, bits=bits, want_bias=True)
    assert torch.equal(gw, gw0) and torch.equal(gb, gb0)
    gw_nb, none = dense.wgrad_bf16_ex2(gy, u, bits=bits, want_bias=False)
    assert none is None and torch.equal(gw_nb, gw0)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 257, 4099, 70001])
@pytest.mark.parametrize("with_bits,bias", [(False, True), (False, False), (True, True)])
def test_weight_gradient_with_the_auxiliary_logit_rows(n, with_bits, bias, device):
    """PMA's four folded-logit rows inside the value projection's weight-gradient pass: the main block is bit-identical to the
    pass without them, the four rows match float64 on the bf16-rounded g4."""
    from allset_amd import dense
    g = torch.Generator().manual_seed(n * 19 + with_bits + 2 * bias)
    O = I = 256
    u, gy = bf(torch.randn(n, I, generator=g), device), bf(torch.randn(n, O, generator=g), device)
    g4 = torch.randn(n, 4, generator=g).to(device)
    bits = None
    if with_bits:
        Wf = bf(torch.randn(O, I, generator=g) / 16, device)
        _, bits = dense.linear_bf16_fwd_mask(u, Wf, None)
    gw0, gb0 = dense.wgrad_bf16_ex2(gy, u, bits=bits, want_bias=bias)
    gw, gb, gwa, gba = dense.wgrad_bf16_ex2(gy, u, bits=bits, g4=g4, want_bias=bias)
    assert torch.equal(gw, gw0) and (gb is None if not bias else torch.equal(gb, gb0))
    g16 = g4.to(torch.bfloat16).double()
    ref_w, ref_b = g16.t() @ u.double(), g16.sum(0)
    assert_one_rounding(gwa, ref_w.cpu(), "gWa")
    assert_one_rounding(gba, ref_b.cpu(), "gba")


@pytest.mark.parametrize("H,C,K,bias", [(4, 64, 256, True), (4, 32, 128, True), (1, 128, 128, False), (2, 64, 256, True), (8, 16, 64, True)])
def test_pma_fold_bf16_against_float64(H, C, K, bias, device):
    from allset_amd import dense
    g = torch.Generator().manual_seed(H * 100 + C + K)
    Wk, bk, att = bf(torch.randn(H * C, K, generator=g) / K ** 0.5, device), (bf(torch.randn(H * C, generator=g), device) if bias else None), \
        bf(torch.randn(1, H, C, generator=g), device)
    Wk_, att_ = Wk.clone().requires_grad_(True), att.clone().requires_grad_(True)
    bk_ = bk.clone().requires_grad_(True) if bias else None
    w, b = dense.pma_fold(Wk_, bk_, att_)
    assert w.dtype == b.dtype == torch.bfloat16
    Gw, Gb = bf(torch.randn(H, K, generator=g), device), bf(torch.randn(H, generator=g), device)
    ((w.float() * Gw.float()).sum() + (b.float() * Gb.float()).sum()).backward()
    Wd, ad = Wk.double().requires_grad_(True), att.double().requires_grad_(True)
    bd = bk.double().requires_grad_(True) if bias else None
    wr = (Wd.view(H, C, K) * ad.view(H, C, 1)).sum(1)
    br = (bd.view(H, C) * ad.view(H, C)).sum(1) if bias else torch.zeros(H, dtype=torch.float64, device=device)
    ((wr * Gw.double()).sum() + (br * Gb.double()).sum()).backward()
    assert_one_rounding(w, wr.detach().cpu(), "w")
    assert_one_rounding(b, br.detach().cpu(), "b")
    assert_one_rounding(Wk_.grad, Wd.grad.cpu(), "gWk")
    assert_one_rounding(att_.grad, ad.grad.cpu(), "gatt")
    if bias:
        assert_one_rounding(bk_.grad, bd.grad.cpu(), "gbk")


def test_residual_block_node_with_bit_masks_equals_the_activation_masked_node(device, monkeypatch):
    """The rFF + ln1 node of PMA's tail (bf16 regime): with the bit masks every output and gradient is bit-identical to the round-5
    form (masks from the saved activations, masked gradient written and re-read)."""
    from allset_amd import dense
    g = torch.Generator().manual_seed(77)
    n, d = 5000, 256
    mk = lambda *s, sc=1.0: bf(torch.randn(*s, generator=g) * sc, device)
    out, w1, b1, w2, b2, gam, bet = mk(n, d), mk(d, d, sc=1 / 16), mk(d), mk(d, d, sc=1 / 16), mk(d), mk(d), mk(d)
    G = mk(n, d)

    def run():
        ts = [t.clone().requires_grad_(True) for t in (out, w1, b1, w2, b2, gam, bet)]
        y = dense.pma_residual_ff_bf16(*ts, 1e-5, True, 0.0)
        y.backward(G)
        return [y.detach()] + [t.grad for t in ts]
    new = run()
    monkeypatch.setattr(dense, "wgrad_bf16_ex2_supported", lambda *a: False)
    old = run()
    for a, b_ in zip(new, old):
        assert torch.equal(a, b_)
