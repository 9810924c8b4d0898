"""CPU: the cell-row format of the forward Deep Sets gather (include/allset_hip_ext.h) restated in numpy --
``encode_cells`` / ``decode_cells`` are the reference the GPU tests (test_gpu_cell_gather.py, test_gpu_cell_epilogue.py) compare the
kernels with.

A row of 128 fp32 becomes 16 cells of 16 bytes, cell c = dwords {v0, v1, v2, meta}, meta = bytes {col0, col1, col2, k}.  k is the row's
count of occupied columns (bit pattern != 0, so -0.0, NaN, Inf and denormals are values), the same in every cell.  The occupied element
of rank j in column order sits in cell j % 16, slot j / 16, at most 48 of them.  An unused slot holds value bits 0 and the dummy column
128 + c.  k > 48 is an overflow row: the cells hold its first 48 elements, the reader takes the row from the dense table."""
import numpy as np

CELLS, CAP, D, PITCH_DW = 16, 48, 128, 64
KS_FIT = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48)
KS_OVER = (49, 60, 128)


def _bits(x: np.ndarray) -> np.ndarray:
    assert x.dtype == np.float32
    return np.ascontiguousarray(x).view(np.uint32)


def encode_cells(x: np.ndarray) -> np.ndarray:
    """f32[n, 128] -> uint32[n, 64], every byte defined."""
    bits = _bits(x)
    n = bits.shape[0]
    assert bits.shape == (n, D)
    out = np.zeros((n, CELLS, 4), dtype=np.uint32)
    for r in range(n):
        cols = np.flatnonzero(bits[r])
        k = len(cols)
        colb = np.empty((CELLS, 3), dtype=np.uint32)
        colb[:] = (128 + np.arange(CELLS, dtype=np.uint32))[:, None]          # dummy columns
        for j, c in enumerate(cols[:CAP]):
            out[r, j % CELLS, j // CELLS] = bits[r, c]
            colb[j % CELLS, j // CELLS] = c
        out[r, :, 3] = colb[:, 0] | (colb[:, 1] << 8) | (colb[:, 2] << 16) | (np.uint32(k) << 24)
    return out.reshape(n, PITCH_DW)


def cell_fields(cells: np.ndarray):
    """uint32[n, 64] -> (values uint32[n, 16, 3], columns int[n, 16, 3], k int[n, 16])."""
    c = np.ascontiguousarray(cells).view(np.uint32).reshape(-1, CELLS, 4)
    meta = c[:, :, 3]
    cols = np.stack([(meta >> (8 * s)) & 0xFF for s in range(3)], axis=-1).astype(np.int64)
    return c[:, :, :3], cols, (meta >> 24).astype(np.int64)


def decode_cells(cells: np.ndarray, dense: np.ndarray) -> np.ndarray:
    """uint32[n, 64] (+ the dense table, read for overflow rows only) -> f32[n, 128], bit for bit: every slot is scattered into an
    image of 128 + 16 dwords, as the gather kernel does it."""
    vals, cols, k = cell_fields(cells)
    n = vals.shape[0]
    image = np.zeros((n, D + CELLS), dtype=np.uint32)
    for r in range(n):
        image[r, cols[r].reshape(-1)] = vals[r].reshape(-1)
    out = image[:, :D].copy()
    over = k[:, 0] > CAP
    out[over] = _bits(dense)[over]
    return out.view(np.float32)


def make_table(ks, seed: int, specials: bool = True) -> np.ndarray:
    """One row per entry of ``ks`` with exactly that many occupied columns at random positions.  ``specials``: -0.0, NaN, +Inf, -Inf and
    a denormal take the place of some values (they are occupied columns)."""
    rng = np.random.default_rng(seed)
    x = np.zeros((len(ks), D), dtype=np.float32)
    for r, k in enumerate(ks):
        cols = rng.permutation(D)[:k]
        v = rng.standard_normal(k).astype(np.float32)
        v[v == 0] = 1.0
        if specials and k >= 5:
            v[:5] = np.array([-0.0, np.nan, np.inf, -np.inf, 1e-45], dtype=np.float32)
        elif specials and k >= 1 and r % 2 == 0:
            v[0] = -0.0
        x[r, cols] = v
    return x


def _same_bits(a, b) -> bool:
    return np.array_equal(_bits(a), _bits(b))


def test_round_trip_for_rows_that_fit():
    ks = KS_FIT * 3
    x = make_table(ks, seed=1)
    assert ((_bits(x) != 0).sum(1) == np.array(ks)).all()                # -0.0, NaN and the denormal count as occupied
    cells = encode_cells(x)
    assert cells.shape == (len(ks), PITCH_DW) and cells.dtype == np.uint32
    assert _same_bits(decode_cells(cells, np.full_like(x, 7.0)), x)       # the dense table is not read for a row that fits
    _, _, k = cell_fields(cells)
    assert (k == np.array(ks)[:, None]).all()                            # the count, in every cell


def test_rank_j_sits_in_cell_j_mod_16_slot_j_div_16():
    x = make_table((33, 48), seed=2, specials=False)
    vals, cols, _ = cell_fields(encode_cells(x))
    for r in range(2):
        occ = np.flatnonzero(_bits(x)[r])
        for j, c in enumerate(occ):
            assert cols[r, j % CELLS, j // CELLS] == c and vals[r, j % CELLS, j // CELLS] == _bits(x)[r, c]


def test_unused_slots_hold_zero_bits_and_the_cell_s_dummy_column():
    ks = KS_FIT
    vals, cols, _ = cell_fields(encode_cells(make_table(ks, seed=3)))
    for r, k in enumerate(ks):
        for j in range(k, 3 * CELLS):
            assert vals[r, j % CELLS, j // CELLS] == 0 and cols[r, j % CELLS, j // CELLS] == 128 + j % CELLS
        used = [cols[r, j % CELLS, j // CELLS] for j in range(k)]
        assert all(c < 128 for c in used) and used == sorted(used)        # column order
        for s in range(3):                                              # slot s is used by some cell iff k > 16 s
            assert bool((cols[r, :, s] < 128).any()) == (k > CELLS * s)


def test_overflow_rows_keep_k_and_their_first_48_elements():
    x = make_table(KS_OVER + (48,), seed=4)
    cells = encode_cells(x)
    vals, cols, k = cell_fields(cells)
    assert (k == np.array(KS_OVER + (48,))[:, None]).all()
    for r in range(len(KS_OVER)):
        occ = np.flatnonzero(_bits(x)[r])[:CAP]
        assert [cols[r, j % CELLS, j // CELLS] for j in range(CAP)] == occ.tolist()
        assert [vals[r, j % CELLS, j // CELLS] for j in range(CAP)] == _bits(x)[r, occ].tolist()
    other = x.copy()
    other[:len(KS_OVER)] = 7.0                                           # what the decoder reads for the overflow rows
    got = decode_cells(cells, other)
    assert _same_bits(got[:len(KS_OVER)], other[:len(KS_OVER)]) and _same_bits(got[-1], x[-1])


def test_occupancy_is_the_bit_pattern_test():
    x = np.zeros((3, D), dtype=np.float32)
    x[0, [5, 31, 32, 100, 127]] = np.array([-0.0, np.nan, np.inf, -np.inf, 1e-45], dtype=np.float32)
    x[1, 0] = 2.0
    cells = encode_cells(x)
    vals, cols, k = cell_fields(cells)
    assert k[:, 0].tolist() == [5, 1, 0]
    assert cols[0, :5, 0].tolist() == [5, 31, 32, 100, 127] and vals[0, :5, 0].tolist() == _bits(x)[0, [5, 31, 32, 100, 127]].tolist()
    assert cols[1, 0, 0] == 0 and vals[1, 0, 0] == np.float32(2.0).view(np.uint32)
    assert not vals[2].any() and (cols[2] == (128 + np.arange(CELLS))[:, None]).all()
    assert _same_bits(decode_cells(cells, x), x)
