"""GPU: the short-row kernels of the two families the benchmark runs -- segreduce_flat_kernel, pma_fwd_flat_kernel and
pma_bwd_src_flat_kernel, forced with ``variant=2`` -- over the twelve row structures of tests/hop_structures.py (empty, 1 x 1, smaller
than a workgroup, everything in one row / from one source, duplicates, empty runs at both ends, rows on the 64-incidence batch
boundary and around 256) at every width on both sides of a lane-group boundary, and the compacted-CSR launch (``sizes=``: the
kernels' ``row_ids``) on the structure that has long and short rows.

References: the float64 operator seam of oracle/allset_oracle.py, as in tests/test_gpu_ops.py; inputs and references come from
tests/hop_structures.py, where tests/test_hop_structures_host.py vouches for them on the CPU.  Tolerance: ``hop_structures.close``
(rtol 1e-4, atol 1e-4 * max(1, max |want|); one structure's logit gradient takes that rule's ``slack``, derived from the float64
reference alone: hop_structures.FLAT_GALPHA_SLACK); bf16 storage: the rule of tests/test_gpu_ops.py::test_bf16_storage_fp32_accumulate
(inputs rounded to bf16 once, the reference computed from the rounded values: rtol 2e-2, atol 1e-2 * max |want|)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_structures as hs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
NAMES = list(hs.structures())
_INCS, _PMA_REF = {}, {}


def _inc(name, transposed=False):
    if (name, transposed) not in _INCS:
        from allset_amd import Incidence
        n_src, n_dst, ei = hs.structures()[name]
        if transposed:
            n_src, n_dst, ei = n_dst, n_src, ei[::-1].copy()
        _INCS[(name, transposed)] = Incidence.from_edge_index(torch.from_numpy(ei).to(DEV), n_src=n_src, n_dst=n_dst)
    return _INCS[(name, transposed)]


def _dev(t):
    return t.float().to(DEV)


def _pma(name, d, transposed):
    """Inputs and float64 reference of one (structure, width), computed once for the forward and the backward test."""
    if (name, d, transposed) not in _PMA_REF:
        inp = hs.flat_pma_inputs(name, *hs.FLAT_PMA_HC[d], transposed)
        _PMA_REF[(name, d, transposed)] = (inp, hs.flat_pma_reference(inp))
    return _PMA_REF[(name, d, transposed)]


@pytest.mark.parametrize("d", hs.FLAT_WIDTHS)
@pytest.mark.parametrize("name", NAMES)
def test_segreduce_short_row_kernel_vs_float64(name, d):
    from allset_amd import ops
    inp = hs.flat_segreduce_inputs(name, d)
    csr = _inc(name).by_dst
    n_t = inp["n_dst"]
    x = _dev(inp["x"])
    w_csr = _dev(inp["w"]).index_select(0, csr.perm.long()).contiguous()
    for reduce, aggr, weighted in ((0, "add", False), (1, "mean", False), (0, "add", True)):
        got, _ = ops.segreduce(reduce, csr.rowptr, csr.col, w_csr if weighted else None, x, n_t, variant=2)
        hs.close(got, hs.flat_segreduce_reference(inp, inp["x"], aggr, weighted), f"{aggr}{' weighted' if weighted else ''}")
    if d % 8 == 0:
        xb = inp["x"].float().bfloat16()
        got, _ = ops.segreduce(0, csr.rowptr, csr.col, None, xb.to(DEV), n_t, variant=2)
        want = hs.flat_segreduce_reference(inp, xb.double(), "add", False)
        assert got.dtype == torch.bfloat16
        torch.testing.assert_close(got.cpu().double(), want, rtol=2e-2, atol=1e-2 * float(want.abs().max()) if want.numel() else 0.0)


def _check_fwd(got, ref):
    for g, want, what in zip(got, ref[:3], ("out", "m", "l")):
        hs.close(g, want, what)


@pytest.mark.parametrize("d", list(hs.FLAT_PMA_HC))
@pytest.mark.parametrize("name", NAMES)
def test_pma_fwd_short_row_kernel_vs_float64(name, d):
    from allset_amd import ops
    inp, ref = _pma(name, d, False)
    csr = _inc(name).by_dst
    _check_fwd(ops.pma_fwd(csr.rowptr, csr.col, _dev(inp["alpha"]), _dev(inp["V"]), inp["H"], 0.2, inp["n_dst"], variant=2), ref)


@pytest.mark.parametrize("d", list(hs.FLAT_PMA_HC))
@pytest.mark.parametrize("name", NAMES)
def test_pma_bwd_src_short_row_kernel_vs_float64(name, d):
    """The structure's rows are the SOURCE rows here: the backward walks the transposed CSR."""
    from allset_amd import ops
    inp, ref = _pma(name, d, True)
    inc = _inc(name, True)
    alpha, V, G = _dev(inp["alpha"]), _dev(inp["V"]), _dev(inp["G"])
    out, m, l = ops.pma_fwd(inc.by_dst.rowptr, inc.by_dst.col, alpha, V, inp["H"], 0.2, inp["n_dst"], variant=1)
    stats = ops.pma_bwd_stats(out, G, m, l)
    gV, galpha = ops.pma_bwd_src(inc.by_src.rowptr, inc.by_src.col, alpha, V, G, stats, 0.2, variant=2)
    hs.close(gV, ref[3], "gV")
    hs.close(galpha, ref[4], "galpha", slack=hs.flat_pma_galpha_slack(inp) if name in hs.FLAT_GALPHA_SLACK else None)


@pytest.mark.parametrize("d", list(hs.FLAT_PMA_HC))
def test_pma_short_row_kernels_on_a_compacted_csr(d):
    """``sizes=``: the long row goes to the one-wave-per-row kernel, the short rows -- a compacted CSR whose row i is row
    ``short_ids[i]`` of the outputs -- to the short-row kernel, forward and backward."""
    from allset_amd import ops
    name = hs.FLAT_SPLIT_STRUCT
    for transposed in (False, True):
        inp, ref = _pma(name, d, transposed)
        inc = _inc(name, transposed)
        alpha, V, G = _dev(inp["alpha"]), _dev(inp["V"]), _dev(inp["G"])
        csr = inc.by_src if transposed else inc.by_dst
        sizes = ops.size_split(csr.rowptr, csr.col, csr.n_rows, csr.max_deg, threshold=hs.CSR_LONG_T)
        assert sizes is not None and sizes.long_ids.numel() == 1 and sizes.short_ids.numel() == csr.n_rows - 1
        if not transposed:
            _check_fwd(ops.pma_fwd(csr.rowptr, csr.col, alpha, V, inp["H"], 0.2, inp["n_dst"], sizes=sizes), ref)
        else:
            out, m, l = ops.pma_fwd(inc.by_dst.rowptr, inc.by_dst.col, alpha, V, inp["H"], 0.2, inp["n_dst"], variant=1)
            gV, galpha = ops.pma_bwd_src(csr.rowptr, csr.col, alpha, V, G, ops.pma_bwd_stats(out, G, m, l), 0.2, sizes=sizes)
            hs.close(gV, ref[3], "gV")
            hs.close(galpha, ref[4], "galpha")
