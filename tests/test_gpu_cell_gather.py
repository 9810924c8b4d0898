"""GPU: the cell-row forward gather (csrc/segreduce.hip pack_cells_kernel / segreduce_cells_kernel).  The cell
path must be BITWISE the dense one and the mask-row one: every comparison here is an equality of bit patterns (as int32: NaNs are
present)."""
import numpy as np
import pytest
import torch

import test_cell_rows_format as fmt

pytestmark = pytest.mark.gpu

SUM, MEAN = 0, 1
# straddle the 8-incidence sub-step, the 16-incidence step and the 64-incidence batch
LENGTHS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130)
N_ROWS, N_SRC = 41, 70                      # 41 rows: not a multiple of the 4 rows of a workgroup


def _bits(t):
    return t.contiguous().view(torch.int32)


def _timed(fn):
    """(fn's result, the names the kernel timer saw)."""
    from allset_amd import ops
    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        ops.set_kernel_timer(None)
    return out, set(timer.events)


def _formats():
    """The packed format of every direction, to put back with ``_restore``."""
    from allset_amd import functional as AF
    return {d: AF.packed_format(d) for d in (None, "v2e", "e2v")}


def _restore(formats):
    from allset_amd import functional as AF
    AF.set_packed_format(formats[None])
    for d in ("v2e", "e2v"):
        AF.set_packed_format(formats[d], d)


def _source_table(specials) -> np.ndarray:
    """70 rows: every k of the format test five times over, overflow rows mixed in.  ``specials``: False; True (-0.0, NaN, +Inf, -Inf and
    a denormal among the values); "one_nan" (the same without -Inf, so that no sum makes a NaN of its own: every NaN has one payload)."""
    ks = [(fmt.KS_FIT + fmt.KS_OVER)[(3 * i) % 14] for i in range(N_SRC)]
    assert set(ks) == set(fmt.KS_FIT + fmt.KS_OVER)
    x = fmt.make_table(ks, seed=21, specials=bool(specials))
    if specials == "one_nan":
        x[np.isneginf(x)] = np.inf
    return x


def _csr(seed=7):
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(0, 20, (N_ROWS,), generator=g)
    deg[:len(LENGTHS)] = torch.tensor(LENGTHS)
    deg = deg[torch.randperm(N_ROWS - 1, generator=g).tolist() + [N_ROWS - 1]]       # special lengths anywhere but the last row
    rowptr = torch.zeros(N_ROWS + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    col = torch.randint(0, N_SRC, (int(rowptr[-1]),), generator=g).to(torch.int32)   # 70 sources, rows up to 130 long: repeats
    return rowptr, col


@pytest.mark.parametrize("strided", [False, True])
def test_pack_cells_matches_the_numpy_reference(strided, device):
    from allset_amd import ops
    for n in (1, 2, 3, 4, 5, N_SRC):                                      # the wave's four rows, the workgroup's sixteen: tails
        x = _source_table(True)[N_SRC - n:]
        ref = torch.from_numpy(fmt.encode_cells(x).view(np.int32))
        if strided:
            buf = torch.full((n, 192), 3.0, device=device)
            buf[:, :128] = torch.from_numpy(x).to(device)
            xd = buf[:, :128]                                            # ldx = 192 > 128
        else:
            xd = torch.from_numpy(x).to(device)
        got = ops.pack_rows(xd, fmt="cells").cpu()
        assert got.shape == (n, fmt.PITCH_DW) and got.dtype == torch.int32
        assert torch.equal(got, ref), n                                  # every byte is defined, overflow rows included


@pytest.mark.parametrize("reduce", [SUM, MEAN])
@pytest.mark.parametrize("ordered", [False, True])
@pytest.mark.parametrize("specials", [False, True, "one_nan"])
def test_segreduce_cells_is_bitwise_the_dense_and_the_mask_gather(reduce, ordered, specials, device):
    """Against the dense gather on every table.  Against the mask gather on every table but the one where NaNs of two payloads meet in
    one sum (Inf - Inf = 0xffc00000 on this hardware, then a gathered 0x7fc00000): v_add_f32 returns its first operand's NaN, the dense
    kernel adds value + sum and the mask kernel sum + value, so THOSE two differ there in the NaN's sign bit -- measured, 1 element of this
    table -- and the cell gather follows the dense one."""
    from allset_amd import ops
    rowptr, col = _csr()
    assert set(LENGTHS) <= set((rowptr[1:] - rowptr[:-1]).tolist())
    rowptr, col = rowptr.to(device), col.to(device)
    xd = torch.from_numpy(_source_table(specials)).to(device)
    cells, packed = ops.pack_rows(xd, fmt="cells"), ops.pack_rows(xd, fmt="mask")
    side = torch.full_like(xd, 7.0)                                      # only the overflow rows of the side table may be read
    over = (_bits(xd) != 0).sum(1) > fmt.CAP
    side[over] = xd[over]
    for n_t in (N_ROWS, N_ROWS - 1):
        order = torch.randperm(n_t, generator=torch.Generator().manual_seed(n_t)).to(torch.int32).to(device) if ordered else None
        rp = rowptr[:n_t + 1]
        want, _ = ops.segreduce(reduce, rp, col, None, xd, n_t, variant=1, row_order=order)
        got = ops.segreduce_packed(reduce, rp, col, cells, side, n_t, row_order=order, fmt="cells")
        mask = ops.segreduce_packed(reduce, rp, col, packed, xd, n_t, row_order=order, fmt="mask")
        assert torch.equal(_bits(got), _bits(want)), n_t
        if specials is not True:
            assert torch.equal(_bits(got), _bits(mask)), n_t
        else:                                                            # all that may differ: which NaN
            same = _bits(got) == _bits(mask)
            assert bool((same | (torch.isnan(got) & torch.isnan(mask))).all()), n_t
        empty = (rp[1:] - rp[:-1]) == 0
        assert not _bits(got)[empty].any()                               # empty rows write +0
    if reduce == SUM and not ordered and specials is False:                   # and the dense kernel is right about a sum (float64 on the host)
        got = ops.segreduce_packed(SUM, rowptr, col, cells, side, N_ROWS, fmt="cells").cpu().double()
        ref = torch.zeros(N_ROWS, 128, dtype=torch.float64)
        ref.index_add_(0, torch.repeat_interleave(torch.arange(N_ROWS), (rowptr[1:] - rowptr[:-1]).cpu().long()), xd.cpu().double()[col.cpu().long()])
        torch.testing.assert_close(got, ref, rtol=1e-5, atol=1e-5)


def test_a_single_source_row_gathered_many_times(device):
    """Every incidence of a step the same row: the four rows of a load instruction and the images of a sub-step all hold one row."""
    from allset_amd import ops
    x = torch.from_numpy(fmt.make_table((48, 49), seed=5, specials=False)).to(device)
    cells = ops.pack_rows(x, fmt="cells")
    rowptr = torch.tensor([0, 130, 147], dtype=torch.int32, device=device)
    col = torch.cat([torch.zeros(130, dtype=torch.int32), torch.ones(17, dtype=torch.int32)]).to(device)
    want, _ = ops.segreduce(SUM, rowptr, col, None, x, 2, variant=1)
    assert torch.equal(_bits(ops.segreduce_packed(SUM, rowptr, col, cells, x, 2, fmt="cells")), _bits(want))


# ---- dispatch: the hint takes the cell path at the built shape, everything else keeps today's route --------------------------------
def _hypergraph(device, n_v=500, n_e=400, pairs=4000, seed=3):
    rng = np.random.default_rng(seed)
    p = sorted({(int(rng.integers(n_v)), int(rng.integers(n_e))) for _ in range(pairs)} | {(v, v % n_e) for v in range(n_v)})
    return torch.tensor(p, dtype=torch.int64).t().contiguous().to(device), n_v, n_e


@pytest.mark.parametrize("case", ["weights", "max", "min", "bf16", "d64", "unaligned"])
def test_hint_falls_back_outside_the_built_shape(case, device):
    from allset_amd import Incidence
    from allset_amd import functional as AF
    assert AF.packed_gather() and AF.packed_format() == "cells"
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    d = 64 if case == "d64" else 128
    x = torch.relu(torch.randn(n_v, d, device=device)) * (torch.rand(n_v, d, device=device) < 0.5)
    if case == "bf16":
        x = x.to(torch.bfloat16)
    if case == "unaligned":
        x = torch.cat([torch.zeros(n_v, 1, device=device), x], 1)[:, 1:]           # rows start 4 bytes off a 16-byte boundary
        assert x.data_ptr() % 16 != 0
    norm = (torch.rand(ei.shape[1], device=device) + 0.5) if case == "weights" else None
    aggr = case if case in ("max", "min") else "add"
    plain = AF.deepsets_aggregate(x, inc, norm, aggr)
    hinted, names = _timed(lambda: AF.deepsets_aggregate(x, inc, norm, aggr, packed_rows=True))
    assert "pack_rows" not in names and "segreduce_fwd" in names
    assert torch.equal(hinted, plain)


@pytest.mark.parametrize("fmt_name", ["cells", "mask"])
def test_hint_takes_the_packed_path_at_the_built_shape(fmt_name, device):
    from allset_amd import Incidence
    from allset_amd import functional as AF
    ei, n_v, n_e = _hypergraph(device)
    inc = Incidence.from_edge_index(ei, n_src=n_v, n_dst=n_e)
    x = torch.relu(torch.randn(n_v, 128, device=device)) * (torch.rand(n_v, 128, device=device) < 0.5)
    was = _formats()
    AF.set_packed_format(fmt_name)
    try:
        for aggr in ("add", "mean"):
            plain = AF.deepsets_aggregate(x, inc, None, aggr)
            hinted, names = _timed(lambda: AF.deepsets_aggregate(x, inc, None, aggr, packed_rows=True))
            assert "pack_rows" in names and "segreduce_fwd" in names
            assert torch.equal(_bits(hinted), _bits(plain))
    finally:
        _restore(was)


def test_the_format_is_chosen_per_direction():
    """The defaults are what tools/cell_gather_bench.py decided: cell rows over the E->V CSR and where no direction is named, mask
    rows over the V->E CSR; ``set_packed_format`` without a direction sets all of them."""
    from allset_amd import functional as AF
    was = _formats()
    assert was == {None: "cells", "v2e": "mask", "e2v": "cells"}
    try:
        with AF.packed_direction("v2e"):
            assert AF.packed_format() == "mask"
            with AF.packed_direction("e2v"):
                assert AF.packed_format() == "cells"
            assert AF.packed_format() == "mask"
        AF.set_packed_format("cells", "v2e")
        assert _formats() == {None: "cells", "v2e": "cells", "e2v": "cells"}
        AF.set_packed_format("mask")
        assert set(_formats().values()) == {"mask"}
        with pytest.raises(ValueError):
            AF.set_packed_format("dense")
    finally:
        _restore(was)
    assert _formats() == was
