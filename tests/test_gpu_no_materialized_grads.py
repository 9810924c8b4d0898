"""GPU: an autograd Function of ``dense`` whose extra outputs never carry a gradient (the packed rows of ``_FusedNormLinearPacked``, the
row statistics ``_WideNormLinear`` emits) gets ``None`` for them in its backward -- autograd's default would fill a zero tensor of
their shape in every backward call, int32 [n, 64] for the packed rows -- and the same gradients come out as before."""
import pytest
import torch

from test_gpu_cell_epilogue import _assert_same, _conv, _route, _run
from test_gpu_cell_gather import _hypergraph

pytestmark = pytest.mark.gpu

N = 4096


def _record(monkeypatch, cls):
    """Wraps ``cls.backward`` with a recorder that calls through; returns the list of the gradient tuples it saw."""
    seen, orig = [], cls.backward

    def backward(ctx, *grads):
        seen.append(grads)
        return orig(ctx, *grads)

    monkeypatch.setattr(cls, "backward", staticmethod(backward))
    return seen


@pytest.mark.parametrize("fmt_name", ["cells", "mask"])
def test_packed_linear_backward_gets_no_gradient_for_the_packed_rows(fmt_name, device, monkeypatch):
    from allset_amd import Incidence, dense
    ei, n_v, n_e = _hypergraph(device, n_v=N, n_e=3000, pairs=20000)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    conv = _conv(device).train()
    params = list(conv.parameters())
    step = lambda t: conv(t, inc, None, "add")
    x = torch.randn(n_v, 128, device=device)
    seen = _record(monkeypatch, dense._FusedNormLinearPacked)
    with _route(fmt_name, True, "on"):
        on, names = _run(step, params, x)
    assert "pack_rows" not in names and len(seen) == 1, "the Linear wrote the packed rows itself"
    gy, g_packed = seen[0]
    assert g_packed is None and gy is not None and tuple(gy.shape) == (n_v, 128)
    with _route(fmt_name, True, "off"):
        off, names = _run(step, params, x)
    assert "pack_rows" in names and len(seen) == 1
    _assert_same(on, off)


class _Unused(torch.autograd.Function):
    """Takes a tensor into the graph and hands no gradient back for it."""

    @staticmethod
    def forward(ctx, t):
        return t.new_zeros(())

    @staticmethod
    def backward(ctx, g):
        return None


def test_packed_linear_whose_rows_get_no_gradient(device, monkeypatch):
    from allset_amd import dense
    g = torch.Generator().manual_seed(4)
    W = (torch.randn(128, 128, generator=g) / 128 ** 0.5).to(device).requires_grad_(True)
    bias, gamma, beta = [(0.1 * torch.randn(128, generator=g) + one).to(device).requires_grad_(True) for one in (0.0, 1.0, 0.0)]
    x = torch.randn(N, 128, generator=g).to(device).requires_grad_(True)
    other = torch.randn(7, device=device, requires_grad=True)
    seen = _record(monkeypatch, dense._FusedNormLinearPacked)
    rows = dense.fused_norm_linear_packed(x, gamma, beta, W, bias, 1e-5, True, 0.5, True, 0.5, "cells")
    (_Unused.apply(rows._side) + (other * 3.0).sum()).backward()
    assert seen == [(None, None)]
    assert all(t.grad is None for t in (x, W, bias, gamma, beta))
    assert torch.equal(other.grad, torch.full((7,), 3.0, device=device))


def test_wide_linear_backward_gets_no_gradient_for_the_emitted_statistics(device, monkeypatch):
    from allset_amd import dense
    n, d = 257, 256
    assert dense.wide_stats_chain_supported(d, d, True, True, 0.5)
    g = torch.Generator().manual_seed(6)
    W = (torch.randn(d, d, generator=g) / d ** 0.5).to(device).requires_grad_(True)
    bias, gamma, beta = [(0.1 * torch.randn(d, generator=g) + one).to(device).requires_grad_(True) for one in (0.0, 1.0, 0.0)]
    x = torch.randn(n, d, generator=g).to(device).requires_grad_(True)
    seen = _record(monkeypatch, dense._WideNormLinear)
    y, stats_y = dense.fused_norm_linear(x, gamma, beta, W, bias, 1e-5, True, 0.5, True, 0.5, emit_stats=(1e-5, False))
    assert tuple(stats_y.shape) == (n, 2) and not stats_y.requires_grad
    y.backward(torch.ones_like(y))
    assert len(seen) == 1 and seen[0][1] is None and seen[0][0] is not None
    for t in (x, W, bias, gamma, beta):
        assert t.grad is not None and bool(torch.isfinite(t.grad).all())
