"""GPU: the bf16 instantiations of csrc/segreduce.hip and csrc/pma.hip are the fp32 arithmetic rounded ONCE.  On the exact tables of
tests/bf16_cases.py (every product and partial sum exact in fp32 in any order) the stored bits must be ``float64 -> .float() ->
.bfloat16()`` and max / min must name the smallest CSR position among equal values; everything else is held to
``bf16_cases.within_one_rounding`` against float64 on the same bf16-rounded inputs (half a bf16 ulp on top of the fp32 kernels' own
1e-4).  The widths and shapes reach the scalar bf16 path (d or C no multiple of 8, or a row pitch that is none), weighted max / min,
the short-row kernels up to 512 columns and every lane-group width of the packet path; tests/test_bf16_cases_host.py vouches for the
cases from float64 alone.  Each test prints ``max |got - ref| / (ulp/2)`` before it asserts."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bf16_cases as bc  # noqa: E402
from oracle import allset_oracle as oracle  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FLT_MAX = float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def graph(device):
    """The structure's two CSRs as the library builds them, pinned to the host CSR the references walk."""
    from allset_amd import Incidence, _lib
    assert (_lib.SUM, _lib.MEAN, _lib.MAX, _lib.MIN) == (bc.SUM, bc.MEAN, bc.MAX, bc.MIN)
    n_src, n_dst, _ = bc.structure()
    inc = Incidence.from_edge_index(bc.edges().to(device), n_src=n_src, n_dst=n_dst)
    for csr, host in ((inc.by_dst, bc.host_csr(False)), (inc.by_src, bc.host_csr(True))):
        assert csr.rowptr.dtype == torch.int32 and csr.col.dtype == torch.int32
        np.testing.assert_array_equal(csr.rowptr.cpu().numpy(), host.rowptr)
        np.testing.assert_array_equal(csr.col.cpu().numpy(), host.col)
        np.testing.assert_array_equal(csr.perm.cpu().numpy(), host.perm)
    return inc


def _csr(graph, flip):
    """(CSR over the output rows, CSR over the gathered rows) of the structure or of its transpose."""
    return (graph.by_src, graph.by_dst) if flip else (graph.by_dst, graph.by_src)


def _table(x, w, device):
    """``x`` (float64 holding bf16 values) as the bf16 matrix the kernel gathers.  A pitch above the width: a view into a wider buffer
    whose other columns hold NaN -- a kernel that read them would show it.  Returns (view, buffer or None)."""
    xb = x.to(BF16)
    assert torch.equal(xb.double(), x)
    if w.pitch == w.d:
        return xb.to(device), None
    buf = torch.full((x.shape[0], w.pitch), float("nan"), dtype=BF16, device=device)
    buf[:, :w.d] = xb.to(device)
    view = buf[:, :w.d]
    assert view.stride(0) == w.pitch and view.data_ptr() == buf.data_ptr()
    return view, buf


def _weights(graph, w_edge, device):
    return None if w_edge is None else w_edge[graph.by_dst.perm.cpu().long()].float().to(device)


# ---- ops.segreduce ----------------------------------------------------------------------------------------------------------------------
_EXACT = [(r, wt, w, 1) for r in (bc.SUM, bc.MAX, bc.MIN) for wt in (False, True) for w in bc.SEG_WIDTHS] + \
         [(bc.SUM, wt, w, 2) for wt in (False, True) for w in bc.FLAT_WIDTHS]
_NAMES = {bc.SUM: "sum", bc.MEAN: "mean", bc.MAX: "max", bc.MIN: "min"}


def _seg_id(p):
    return "-".join([_NAMES[p[0]], "w" if p[1] else "plain", p[2].id, f"v{p[3]}"] + list(p[4:]))


@pytest.mark.parametrize("case", _EXACT, ids=_seg_id)
def test_segreduce_exact_tables_store_the_expected_bits(case, graph, device):
    from allset_amd import ops
    reduce, weighted, w, variant = case
    ext = reduce in (bc.MAX, bc.MIN)
    x = bc.exact_table(w.d, signed=ext)
    w_edge = bc.exact_weights() if weighted else None
    ref, ref_arg = bc.seg_reference(reduce, x, w_edge)
    want = ref.float().to(BF16)
    csr = graph.by_dst
    xv, buf = _table(x, w, device)
    before = None if buf is None else buf.clone()
    out, arg = ops.segreduce(reduce, csr.rowptr, csr.col, _weights(graph, w_edge, device), xv, csr.n_rows, want_arg=ext, variant=variant)
    assert out.dtype == BF16 and tuple(out.shape) == (csr.n_rows, w.d)
    same = bc.bits_equal(out, want)
    print(f"{_seg_id(case)}: {int((~same).sum())} of {same.numel()} elements differ; max |got - ref| / (ulp/2) = {bc.half_ulps(out, ref):.4f}")
    if not bool(same.all()):
        i = tuple(int(v) for v in (~same).nonzero()[0])
        raise AssertionError(f"{int((~same).sum())} of {same.numel()} elements are not the expected bf16 bits; first at {i} (row length "
                             f"{int(bc.row_lengths()[i[0]])}): got {float(out[i])!r}, float64 {float(ref[i])!r}, expected {float(want[i])!r}")
    empty = torch.from_numpy(bc.row_lengths() == 0)
    assert bool(empty.any()) and bool((out.cpu()[empty].view(torch.int16) == 0).all())              # an empty row is +0
    if ext:
        assert arg.dtype == torch.int32 and torch.equal(arg.cpu(), ref_arg)
        assert bool((arg.cpu()[empty] == -1).all())
    else:
        assert arg is None
    if buf is not None:                                                                                # the gathered buffer is read-only
        assert torch.equal(buf.view(torch.int16), before.view(torch.int16))


_ROUNDED = [(bc.MEAN, wt, w, 1, "exact") for wt in (False, True) for w in bc.SEG_WIDTHS] + \
           [(r, wt, w, 1, "general") for r in (bc.SUM, bc.MEAN) for wt in (False, True) for w in bc.SEG_WIDTHS] + \
           [(bc.MEAN, wt, w, 2, "exact") for wt in (False, True) for w in bc.FLAT_WIDTHS] + \
           [(r, wt, w, 2, "general") for r in (bc.SUM, bc.MEAN) for wt in (False, True) for w in bc.FLAT_WIDTHS]


@pytest.mark.parametrize("case", _ROUNDED, ids=_seg_id)
def test_segreduce_is_one_rounding_from_float64(case, graph, device):
    from allset_amd import ops
    reduce, weighted, w, variant, table = case
    if table == "exact":
        x, w_edge = bc.exact_table(w.d), (bc.exact_weights() if weighted else None)
    else:
        x, w_edge = bc.general_table(bc.N_SRC, w.d), (bc.general_weights() if weighted else None)
    ref, _ = bc.seg_reference(reduce, x, w_edge)
    csr = graph.by_dst
    xv, _ = _table(x, w, device)
    wd = _weights(graph, w_edge, device)
    out, _ = ops.segreduce(reduce, csr.rowptr, csr.col, wd, xv, csr.n_rows, variant=variant)
    assert out.dtype == BF16
    bc.assert_one_rounding(out, ref, _seg_id(case))
    if variant == 1:                                                       # a processing order moves no bit
        order = torch.from_numpy(np.random.default_rng(7).permutation(csr.n_rows).astype(np.int32)).to(device)
        again, _ = ops.segreduce(reduce, csr.rowptr, csr.col, wd, xv, csr.n_rows, variant=1, row_order=order)
        assert torch.equal(again.view(torch.int16), out.view(torch.int16))


# ---- backward of the bf16 Deep Sets aggregation: the transposed gather in bf16 -----------------------------------------------------------
@pytest.mark.parametrize("with_norm", [False, True], ids=["plain", "norm"])
@pytest.mark.parametrize("d", bc.BWD_WIDTHS)
@pytest.mark.parametrize("aggr", ["add", "mean"])
def test_deepsets_aggregate_bf16_forward_and_backward(aggr, d, with_norm, graph, device):
    from allset_amd import deepsets_aggregate
    n_src, n_dst, _ = bc.structure()
    ei = bc.edges()
    x, G = bc.general_table(n_src, d), bc.general_table(n_dst, d, "G")
    norm = bc.general_weights() if with_norm else None
    xo = x.clone().requires_grad_(True)
    ref = oracle.deepsets_aggregate(xo, ei, norm if with_norm else torch.ones(ei.shape[1], dtype=bc.D64), aggr)
    ref = torch.cat([ref, ref.new_zeros(n_dst - ref.shape[0], d)])
    (ref * G).sum().backward()

    xg = x.to(BF16).to(device).requires_grad_(True)
    out = deepsets_aggregate(xg, graph, norm.float().to(device) if with_norm else None, aggr)
    out.backward(G.to(BF16).to(device))
    assert out.dtype == BF16 and xg.grad.dtype == BF16
    what = f"deepsets {aggr} d{d} {'norm' if with_norm else 'plain'}"
    bc.assert_one_rounding(out, ref.detach(), what + " out")
    bc.assert_one_rounding(xg.grad, xo.grad, what + " x.grad")
    isolated = torch.from_numpy(bc.row_lengths(True) == 0)
    assert bool((xg.grad.cpu()[isolated].view(torch.int16) == 0).all())


# ---- ops.pma_fwd, ops.pma_bwd_stats, ops.pma_bwd_src --------------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [False, True], ids=["rows-long", "rows-short"])
@pytest.mark.parametrize("shape", bc.PMA_SHAPES, ids=lambda s: s.id)
def test_pma_kernels_are_one_rounding_from_float64(shape, flip, graph, device):
    """Each entry against float64 on ITS OWN inputs.  ``pma_fwd``: ``out`` (bf16), ``m``, ``l``.  ``pma_bwd_stats`` reads the STORED bf16
    ``out``, so its reference ``<out, G>`` is formed from those stored values.  ``pma_bwd_src`` is handed the float64 statistics of the
    unrounded pooling (as fp32), so that ``gV`` (bf16) and ``galpha`` are the oracle's autograd gradients; through the stored ``out`` the
    statistic, and ``galpha`` with it, carries the storage rounding -- 2^-9 relative per element of ``out``, the regime's accuracy and
    not the arithmetic's -- which the fp32 tolerance of this test must not absorb.  ``flip``: the transposed structure, where the
    forward walks the short rows and the backward the long ones."""
    from allset_amd import ops
    H, C, variant = shape.H, shape.C, shape.variant
    r = bc.pma_reference(H, C, flip)
    fwd, bwd = _csr(graph, flip)
    n_t, n_s = r["n_t"], r["n_s"]
    assert (fwd.n_rows, bwd.n_rows) == (n_t, n_s)
    V, G = r["V"].to(BF16).to(device), r["G"].to(BF16).to(device)
    alpha = r["alpha"].float().to(device)
    what = f"pma {shape.id} {'rows-short' if flip else 'rows-long'}"
    empty = r["empty"]

    out, m, l = ops.pma_fwd(fwd.rowptr, fwd.col, alpha, V, H, bc.PMA_SLOPE, n_t, variant=variant)
    assert out.dtype == BF16 and m.dtype == torch.float32 and l.dtype == torch.float32
    bc.assert_one_rounding(out, r["out"], what + " out")
    bc.close_fp32(m, r["m"], what + " m")
    bc.close_fp32(l, r["l"], what + " l")
    assert bool((out.cpu()[empty].view(torch.int16) == 0).all()) and bool((m.cpu()[empty] == 0).all()) and bool((l.cpu()[empty] == 0).all())

    stats = ops.pma_bwd_stats(out, G, m, l)
    assert stats.dtype == torch.float32 and tuple(stats.shape) == (n_t, H, 2)
    want = bc.pma_stats_reference(out.cpu().double(), r["G"], m.cpu().double(), l.cpu().double(), H)
    got = stats.cpu()
    bc.close_fp32(got[~empty][..., 0], want[~empty][..., 0], what + " stats M")
    bc.close_fp32(got[..., 1], want[..., 1], what + " stats delta")
    assert bool((got[empty][..., 0] == FLT_MAX).all())                     # an empty row: exp(a - FLT_MAX) = 0 for whoever gathers it

    st = r["stats"].clone()
    st[empty, :, 0] = FLT_MAX
    gV, galpha = ops.pma_bwd_src(bwd.rowptr, bwd.col, alpha, V, G, st.float().to(device), bc.PMA_SLOPE, variant=variant)
    assert gV.dtype == BF16 and galpha.dtype == torch.float32
    bc.assert_one_rounding(gV, r["gV"], what + " gV")
    bc.close_fp32(galpha, r["galpha"], what + " galpha")


@pytest.mark.parametrize("H,C", bc.PMA_SCALAR)
def test_pma_short_row_variant_is_refused_on_scalar_shapes(H, C, graph, device):
    """C % 8 != 0 in bf16: a forced short-row variant is the entry's error, not a quiet run of the other kernel."""
    from allset_amd import ops
    from allset_amd._lib import AllSetHipError
    r = bc.pma_reference(H, C, False)
    fwd, bwd = _csr(graph, False)
    V, G = r["V"].to(BF16).to(device), r["G"].to(BF16).to(device)
    alpha = r["alpha"].float().to(device)
    with pytest.raises(AllSetHipError, match="the short-row variant needs"):
        ops.pma_fwd(fwd.rowptr, fwd.col, alpha, V, H, bc.PMA_SLOPE, r["n_t"], variant=2)
    with pytest.raises(AllSetHipError, match="the short-row variant needs"):
        ops.pma_bwd_src(bwd.rowptr, bwd.col, alpha, V, G, r["stats"].float().to(device), bc.PMA_SLOPE, variant=2)
