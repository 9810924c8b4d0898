"""GPU: the cell-row epilogue of the fused Linear (csrc/fused_fwd2.hip mode 4) stages a row's occupied elements in rank order and lets
lane c build cell c from ranks c, 16 + c and 32 + c.  The cases walk the row's count k across the places where that can go wrong -- no
element, the first element of the second and of the third slot, the cap of 48 from both sides, every row above it -- at row counts
around the 32-row stage, in both arithmetics, against ``ops.pack_rows(dense.fused_linear_fwd(...), fmt="cells")``.  Every comparison is
an equality of bit patterns."""
import pytest
import torch

import test_cell_rows_format as fmt
from test_gpu_cell_gather import _bits

pytestmark = pytest.mark.gpu

ROWS = (1, 31, 32, 33, 100)                 # a partial stage; one row short of a stage; exactly one; one stage plus one row; three and a bit
# m columns carry a bias of +6, the others -6, against Linear terms of standard deviation < 0.1: a +6 column is occupied exactly when the
# output dropout (p = 0.5) keeps it, so k ~ Binomial(m, 1/2) -- and the k each m is there for (over the 197 rows of ROWS, each n under its
# own dropout seed; the rarest, k = 49 at m = 96, has probability 0.078 per row: absent with probability 1e-7)
M_KS = {0: (0,), 2: (0, 1, 2), 34: (16, 17), 64: (32, 33), 96: (48, 49), 128: ()}
ARITHS = ("auto", "strict")


def _params(m, device):
    g = torch.Generator().manual_seed(23)
    W = 0.25 * torch.randn(128, 128, generator=g) / 128 ** 0.5
    gamma = 1.0 + 0.1 * torch.randn(128, generator=g)
    beta = 0.1 * torch.randn(128, generator=g)
    bias = torch.full((128,), -6.0)
    bias[:m] = 6.0
    return [t.to(device) for t in (W, bias, gamma, beta)]


def _special_params(device):
    """A Linear without a relu behind it whose output holds NaN, Inf, -0.0 and exact +0.0: columns 0..69 bias +6 (12.0 kept, +0.0
    dropped), 70..73 bias -6 (-12.0 kept, -0.0 dropped: occupied either way), 74..76 bias +Inf (Inf kept, Inf * 0 = NaN dropped), 77..78
    bias NaN, the rest a zero weight row and a zero bias (+0.0 whatever the dropout does): k = 9 + Binomial(70, 1/2), both sides of 48."""
    W, bias, gamma, beta = _params(70, device)
    bias[74:77] = float("inf")
    bias[77:79] = float("nan")
    bias[79:] = 0.0
    W[79:] = 0.0
    return W, bias, gamma, beta


def _csr(n_src, device):
    """300 incidences over 21 rows: an empty row, a row of 38, the rest between 4 and 37."""
    g = torch.Generator().manual_seed(5)
    deg = [0, 38] + [13] * 19
    deg[2:] = [13 + d for d in (torch.randperm(19, generator=g) - 9).tolist()]
    deg[-1] += 300 - sum(deg)
    assert sum(deg) == 300 and min(deg[1:]) >= 1 and deg[0] == 0 and deg[1] == 38
    rowptr = torch.zeros(len(deg) + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(torch.tensor(deg), 0).to(torch.int32)
    col = torch.randint(0, n_src, (300,), generator=g).to(torch.int32)
    return rowptr.to(device), col.to(device), len(deg)


def _compare(params, relu_out, arith, device):
    """Both routes at every row count; returns every row's k.  The last row count is also gathered."""
    from allset_amd import dense, ops
    W, bias, gamma, beta = params
    ks = []
    for n in ROWS:
        x = torch.randn(n, 128, generator=torch.Generator().manual_seed(n)).to(device)
        words = dense.activation_mask_words(n, 128)
        m_ref = torch.zeros(words, dtype=torch.int32, device=device)
        m_new = torch.zeros(words, dtype=torch.int32, device=device)
        seeds = (101, 202 + n)
        with dense.arithmetic(arith):
            y, stats = dense.fused_linear_fwd(x, W, bias, gamma, beta, 1e-5, True, 0.5, seeds[0], relu_out, 0.5, seeds[1], None, m_ref)
            cells, side, stats_new = ops.fused_linear_fwd_packed(x, W, bias, gamma, beta, 1e-5, True, 0.5, seeds[0], relu_out, 0.5, seeds[1],
                                                                 None, m_new, dense._arith_for(0, 128, 128, True, 0), fmt="cells")
        k = (_bits(y) != 0).sum(1)
        ks.append(k.cpu())
        assert torch.equal(cells, ops.pack_rows(y, fmt="cells")), (n, "cell rows")
        over = k > fmt.CAP
        assert torch.equal(_bits(side)[over], _bits(y)[over]), (n, "side table on the rows above the cap")
        assert torch.equal(m_new, m_ref), (n, "1-bit activation mask")
        assert torch.equal(_bits(stats_new), _bits(stats)), (n, "row statistics")
    rowptr, col, n_t = _csr(ROWS[-1], device)
    want, _ = ops.segreduce(0, rowptr, col, None, y, n_t, variant=1)
    got = ops.segreduce_packed(0, rowptr, col, cells, side, n_t, fmt="cells")
    assert torch.equal(_bits(got), _bits(want)), "the gather over the epilogue's rows"
    return torch.cat(ks)


@pytest.mark.parametrize("m", sorted(M_KS))
@pytest.mark.parametrize("arith", ARITHS)
def test_cell_rows_in_rank_order_equal_linear_then_pack(arith, m, device):
    from allset_amd import dense, ops
    params = _params(m, device)
    # the class holds what it is there for -- from the dense route alone, before anything is compared
    seen = set()
    for n in ROWS:
        x = torch.randn(n, 128, generator=torch.Generator().manual_seed(n)).to(device)
        with dense.arithmetic(arith):
            y, _ = dense.fused_linear_fwd(x, *params, 1e-5, True, 0.5, 101, True, 0.5, 202 + n, None, None)
        seen |= set((_bits(y) != 0).sum(1).tolist())
    print(f"m={m} {arith}: k in {sorted(seen)}")
    assert set(M_KS[m]) <= seen, (m, sorted(seen))
    if m == 0:
        assert seen == {0}
    if m == 128:                                 # Binomial(128, 1/2): P(k <= 48) = 0.003 per row
        assert min(seen) > 40 and sum(k > fmt.CAP for k in seen) >= len(seen) - 2
    k = _compare(params, True, arith, device)
    assert set(k.tolist()) == seen
    assert ops.fused_linear_fwd_packed_supported(128, 128, True, 0.5, 0.5, fmt="cells")


@pytest.mark.parametrize("arith", ARITHS)
def test_nan_inf_and_negative_zero_are_values(arith, device):
    from allset_amd import dense
    params = _special_params(device)
    x = torch.randn(ROWS[-1], 128, generator=torch.Generator().manual_seed(ROWS[-1])).to(device)
    with dense.arithmetic(arith):
        y, _ = dense.fused_linear_fwd(x, *params, 1e-5, True, 0.5, 101, False, 0.5, 202 + ROWS[-1], None, None)
    b = _bits(y)
    assert bool(torch.isnan(y).any()) and bool(torch.isinf(y).any()) and bool((b == -2 ** 31).any()) and bool((b == 0).any())
    assert bool((b[:, 70:79] != 0).all()), "-0.0, NaN and Inf count as occupied"
    k = _compare(params, False, arith, device)
    print(f"specials {arith}: k min {int(k.min())} max {int(k.max())}")
    assert int(k.min()) <= fmt.CAP < int(k.max())
