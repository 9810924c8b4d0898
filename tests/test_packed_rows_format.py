"""CPU: the packed-nonzero-row format of the forward Deep Sets gather (include/allset_hip_ext.h) restated in
plain torch -- ``encode_rows`` / ``decode_rows`` are the reference the GPU tests (test_gpu_packed_gather.py) compare the kernels with.

A row of 128 fp32 becomes 64 dwords: dwords 0..3 a 128-bit occupancy mask (bit c set iff the BIT PATTERN of element c is not zero, so
-0.0, NaN and Inf are values), dwords 4..4+k-1 the k occupied elements in column order, bit for bit.  A row with k > 60 is an overflow
row: full mask, values unspecified, the reader takes the row from the dense table."""
import torch

PITCH_DW, CAP, D = 64, 60, 128
KS = (0, 1, 59, 60, 61, 128)


def _occupancy(bits: torch.Tensor) -> torch.Tensor:
    return bits != 0


def encode_rows(x: torch.Tensor) -> torch.Tensor:
    """f32[n, 128] -> int32[n, 64].  Unspecified dwords (behind the values; every value dword of an overflow row) are zero here."""
    assert x.dtype == torch.float32 and x.dim() == 2 and x.shape[1] == D
    bits = x.contiguous().view(torch.int32)
    occ = _occupancy(bits)
    n = x.shape[0]
    packed = torch.zeros(n, PITCH_DW, dtype=torch.int32)
    weights = torch.ones(32, dtype=torch.int64) << torch.arange(32, dtype=torch.int64)
    m = (occ.view(n, 4, 32).to(torch.int64) * weights).sum(-1)
    packed[:, :4] = torch.where(m >= 2 ** 31, m - 2 ** 32, m).to(torch.int32)
    fits = occ.sum(1) <= CAP
    pos = torch.cumsum(occ, 1) + 3                                   # dword of each occupied element: 4 + (occupied columns below)
    rows, cols = torch.nonzero(occ & fits[:, None], as_tuple=True)
    packed[rows, pos[rows, cols]] = bits[rows, cols]
    return packed


def mask_bits(packed: torch.Tensor) -> torch.Tensor:
    """bool[n, 128]: the occupancy the mask dwords state."""
    m = packed[:, :4].to(torch.int64) & 0xFFFFFFFF
    return (((m[:, :, None] >> torch.arange(32, dtype=torch.int64)) & 1) != 0).reshape(packed.shape[0], D)


def decode_rows(packed: torch.Tensor, dense: torch.Tensor) -> torch.Tensor:
    """int32[n, 64] (+ the dense table, read for overflow rows only) -> f32[n, 128], bit for bit."""
    occ = mask_bits(packed)
    fits = occ.sum(1) <= CAP
    pos = torch.cumsum(occ, 1) + 3
    out = torch.zeros(packed.shape[0], D, dtype=torch.int32)
    rows, cols = torch.nonzero(occ & fits[:, None], as_tuple=True)
    out[rows, cols] = packed[rows, pos[rows, cols]]
    out[~fits] = dense.contiguous().view(torch.int32)[~fits]
    return out.view(torch.float32)


def make_table(ks, seed: int, specials: bool = True, sign: float = 0.0) -> torch.Tensor:
    """One row per entry of ``ks`` with exactly that many occupied columns at random positions.  ``specials``: -0.0, NaN, +Inf and
    -Inf take the place of some values (they are occupied columns).  ``sign`` < 0: every value negative."""
    g = torch.Generator().manual_seed(seed)
    n = len(ks)
    x = torch.zeros(n, D)
    for r, k in enumerate(ks):
        cols = torch.randperm(D, generator=g)[:k]
        v = torch.randn(k, generator=g)
        v = torch.where(v == 0, torch.ones_like(v), v)
        if sign < 0:
            v = -v.abs()
        if specials and k >= 4:
            v[:4] = torch.tensor([-0.0, float("nan"), float("inf"), float("-inf")])
        elif specials and k >= 1 and r % 2 == 0:
            v[0] = -0.0
        x[r, cols] = v
    return x


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_round_trip_over_the_capacity_edge():
    x = make_table(KS * 3, seed=1)
    assert (_occupancy(x.view(torch.int32)).sum(1) == torch.tensor(KS * 3)).all()      # -0.0 and NaN count as occupied
    packed = encode_rows(x)
    assert packed.shape == (len(KS) * 3, PITCH_DW) and packed.dtype == torch.int32
    assert _same_bits(decode_rows(packed, x), x)


def test_mask_is_the_bit_pattern_test():
    x = torch.zeros(3, D)
    x[0, 5], x[0, 31], x[0, 32], x[0, 127] = -0.0, float("nan"), float("inf"), 1e-45      # a denormal is a value too
    x[1, 0] = 2.0
    packed = encode_rows(x)
    occ = mask_bits(packed)
    assert occ[0].nonzero().flatten().tolist() == [5, 31, 32, 127] and occ[1].nonzero().flatten().tolist() == [0]
    assert not occ[2].any() and not packed[2].any()
    assert packed[0, :4].tolist() == [(1 << 5) - (1 << 31), 1, 0, -(1 << 31)]
    assert packed[0, 4:8].tolist() == x[0, [5, 31, 32, 127]].view(torch.int32).tolist()
    assert packed[1, 4].item() == torch.tensor(2.0).view(torch.int32).item()


def test_values_sit_in_column_order_behind_the_mask():
    x = make_table((59, 60), seed=2, specials=False)
    packed = encode_rows(x)
    for r, k in enumerate((59, 60)):
        cols = _occupancy(x[r].view(torch.int32)).nonzero().flatten()
        assert packed[r, 4:4 + k].tolist() == x[r, cols].view(torch.int32).tolist()
        assert not packed[r, 4 + k:].any()


def test_overflow_rows_come_from_the_dense_table():
    x = make_table((61, 128, 60), seed=3)
    packed = encode_rows(x)
    assert (mask_bits(packed).sum(1) == torch.tensor([61, 128, 60])).all()            # the mask is written in full
    other = x.clone()
    other[:2] = 7.0                                                                   # what the decoder reads for rows 0 and 1
    got = decode_rows(packed, other)
    assert _same_bits(got[:2], other[:2]) and _same_bits(got[2], x[2])
