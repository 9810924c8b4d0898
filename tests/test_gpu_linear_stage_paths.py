"""The stage paths of the fused Linear kernels at d = 128 (csrc/fused_fwd2.hip, csrc/fused_bwd6.hip / fused_bwd4.hip): a workgroup
walks its 32-row stages blockIdx.x, blockIdx.x + grid, ...; the main trips run full stages from running addresses, the edges (the
first stage, the last few, a partial last one) run the general code.  Row counts around every boundary of that walk, every operand
layout the entries accept, both arithmetics.

(a) Rows are independent and the dropout hash is keyed by (row, column): every row-wise output of a call on n rows must be BITWISE the
    first n rows of a call on more rows, the extra rows random, the same seeds.  Two larger calls: the next multiple of 32 * grid
    above n (the same rows in full stages, the partial one gone), and 8 * 32 * grid rows -- a workgroup's main trips start at five
    stages (two stages per trip, requests two stages ahead), so only there do the rows that the small call walks with the general
    code (at most four stages per workgroup) go through the main trips.
(b) The column sums (gW, gb, dgamma, dbeta) against the float64 restatement of the dense tests, under the rule of tests/util.py
    ``close``: rtol, and atol relative to the expected tensor's largest magnitude."""
import pytest
import torch

pytestmark = pytest.mark.gpu

D = 128
EPS = 1e-5
P_IN, P_OUT = 0.5, 0.25
SEED_IN, SEED_OUT = 4242, 977
BLOCKS = (4, 8, 16, 32, 64)
RTOL = ATOL = 2e-5          # tests/test_oracle_golden.py's bound for fp32 against float64 (fp32 sums of <= 32768 terms stay far below it)


def _grid():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _row_counts():
    g = _grid()
    return [1, 31, 32, 33, 64, 65, 32 * g - 1, 32 * g, 32 * g + 1, 32 * (g + 1), 32 * (g + 1) + 1, 3 * 32 * g + 17]


ROW_CASES = list(range(12))          # indices into _row_counts() (the counts depend on the device)


@pytest.fixture
def arith_mode(request):
    from allset_amd import dense
    prev = dense.set_arithmetic(request.param)
    yield request.param
    dense.set_arithmetic(prev)


BOTH_ARITH = pytest.mark.parametrize("arith_mode", ["auto", "strict"], indirect=True)


def close(got, exp, what):
    """tests/util.py ``close`` (nested there): atol relative to the largest magnitude of the expected tensor"""
    scale = float(exp.abs().max()) if exp.numel() else 0.0
    torch.testing.assert_close(got.to(exp.dtype), exp, rtol=RTOL, atol=ATOL * max(scale, 1e-3), msg=lambda m: f"{what}: {m}")


def to_blocked(t, cb):
    n, C = t.shape
    return t.view(n, C // cb, cb).permute(1, 0, 2).reshape(-1, cb).contiguous()


def from_blocked(t, cb, C=D):
    n = t.shape[0] // (C // cb)
    return t.view(C // cb, n, cb).permute(1, 0, 2).reshape(n, C)


def wide(t):
    """the same [n, 128] values as a view of a [n, 160] tensor (ld = 160)"""
    w = torch.randn(t.shape[0], 160, device=t.device)
    w[:, :D] = t
    return w[:, :D]


def mask_words_of_rows(n, device):
    """indices of the mask dwords that belong to rows < n ("mask layout", include/allset_hip.h: block (row / 16, column / 64) of 32
    dwords, dword (row % 16, 32-column group))"""
    r = torch.arange(n, device=device).view(-1, 1, 1)
    hb = torch.arange(2, device=device).view(1, -1, 1)
    g = torch.arange(2, device=device).view(1, 1, -1)
    return ((((r // 16) * 2 + hb) * 32) + ((r % 16) // 4) * 8 + (r % 4) * 2 + g).reshape(-1)


def same(a, b, what):
    assert torch.equal(a, b), f"{what}: {(a != b).sum().item()} of {a.numel()} elements differ"


def _params(gen, device):
    W = (torch.randn(D, D, generator=gen) / D ** 0.5).to(device)
    b = (0.1 * torch.randn(D, generator=gen)).to(device)
    gamma = (1 + 0.2 * torch.randn(D, generator=gen)).to(device)
    beta = (0.3 * torch.randn(D, generator=gen)).to(device)
    return W, b, gamma, beta


def _sizes(case):
    """n, and the row counts of the larger calls"""
    n = _row_counts()[case]
    step = 32 * _grid()
    return n, ((n // step + 1) * step, 8 * step)


@BOTH_ARITH
@pytest.mark.parametrize("case", ROW_CASES)
def test_forward_rows_do_not_depend_on_the_stage_path(case, arith_mode, device):
    from allset_amd import dense, ops
    n, larger = _sizes(case)
    gen = torch.Generator().manual_seed(100 + case)
    W, b, gamma, beta = _params(gen, device)
    X = (torch.randn(max(larger), D, generator=gen) * 2 + 0.3).to(device)
    assert dense.blocked_linear_supported(D, D)

    def light(x, xcb=0, ycb=0):
        if xcb or ycb:
            y, st = dense.fused_linear_fwd_blocked(to_blocked(x, xcb) if xcb else x, xcb, W, b, gamma, beta, EPS, False, 0.0, 0, False, 0.0, 0,
                                                   None, None, ycb)
            return (from_blocked(y, ycb) if ycb else y), st, None
        y, st = dense.fused_linear_fwd(x, W, b, gamma, beta, EPS, False, 0.0, 0, False, 0.0, 0)
        return y, st, None

    def heavy(x, xcb=0, ycb=0):
        rows = x.shape[0]
        mask = torch.zeros(dense.activation_mask_words(rows, D), dtype=torch.int32, device=device)
        if xcb or ycb:
            y, st = dense.fused_linear_fwd_blocked(to_blocked(x, xcb) if xcb else x, xcb, W, b, gamma, beta, EPS, True, P_IN, SEED_IN, True,
                                                   P_OUT, SEED_OUT, None, mask, ycb)
            return (from_blocked(y, ycb) if ycb else y), st, mask
        y, st = dense.fused_linear_fwd(x, W, b, gamma, beta, EPS, True, P_IN, SEED_IN, True, P_OUT, SEED_OUT, None, mask)
        return y, st, mask

    layouts = [("row-major", lambda x: x, 0, 0), ("ld=160", wide, 0, 0)]
    layouts += [(f"x blocked by {cb}", lambda x: x, cb, 0) for cb in BLOCKS] + [(f"y blocked by {cb}", lambda x: x, 0, cb) for cb in BLOCKS]
    words = mask_words_of_rows(n, device)
    for kind, fn in (("light", light), ("heavy", heavy)):
        for name, view, xcb, ycb in layouts:
            y_n, st_n, m_n = fn(view(X[:n]), xcb, ycb)
            for N in larger:
                y_N, st_N, m_N = fn(view(X[:N]), xcb, ycb)
                same(y_n, y_N[:n], f"{kind} forward, {name}, {n} of {N} rows: y")
                same(st_n, st_N[:n], f"{kind} forward, {name}, {n} of {N} rows: row statistics")
                if m_n is not None:
                    same(m_n[words], m_N[words], f"{kind} forward, {name}, {n} of {N} rows: 1-bit mask")

    # modes 3 and 4: the packed-row epilogues (LayerNorm prologue, relu and both dropouts; row-major x)
    arith = dense._arith_for(0, D, D, True, 0)
    for fmt in ("mask", "cells"):
        if not ops.fused_linear_fwd_packed_supported(D, D, True, P_IN, P_OUT, fmt=fmt):
            pytest.fail(f"the packed forward ({fmt}) is not built for 128 x 128")
        for name, view in (("row-major", lambda x: x), ("ld=160", wide)):
            out = []
            for x in (view(X[:n]),) + tuple(view(X[:N]) for N in larger):
                mask = torch.zeros(dense.activation_mask_words(x.shape[0], D), dtype=torch.int32, device=device)
                packed, _side, st = ops.fused_linear_fwd_packed(x, W, b, gamma, beta, EPS, True, P_IN, SEED_IN, True, P_OUT, SEED_OUT, None,
                                                                mask, arith, fmt=fmt)
                out.append((packed, st, mask))
            p_n, st_n, m_n = out[0]
            for N, (p_N, st_N, m_N) in zip(larger, out[1:]):
                same(p_n, p_N[:n], f"packed forward ({fmt}), {name}, {n} of {N} rows: packed rows")
                same(st_n, st_N[:n], f"packed forward ({fmt}), {name}, {n} of {N} rows: row statistics")
                same(m_n[words], m_N[words], f"packed forward ({fmt}), {name}, {n} of {N} rows: 1-bit mask")


@BOTH_ARITH
@pytest.mark.parametrize("case", ROW_CASES)
def test_backward_rows_and_column_sums_on_every_stage_path(case, arith_mode, device):
    from allset_amd import dense
    n, larger = _sizes(case)
    gen = torch.Generator().manual_seed(200 + case)
    W, b, gamma, beta = _params(gen, device)
    X = (torch.randn(max(larger), D, generator=gen) * 2 + 0.3).to(device)
    G = torch.randn(max(larger), D, generator=gen).to(device)

    # what the heavy backward needs from its forward: the row statistics of relu(x), the 1-bit mask of y > 0 (one mask per row count)
    masks = {}
    for rows in (n,) + larger:
        masks[rows] = torch.zeros(dense.activation_mask_words(rows, D), dtype=torch.int32, device=device)
        y_N, st_heavy = dense.fused_linear_fwd(X[:rows], W, b, gamma, beta, EPS, True, P_IN, SEED_IN, True, P_OUT, SEED_OUT, None, masks[rows])
    _, st_light = dense.fused_linear_fwd(X, W, b, gamma, beta, EPS, False, 0.0, 0, False, 0.0, 0)

    def light(g, x, rows, gcb=0, xcb=0):
        if gcb or xcb:
            r = dense.fused_linear_bwd_all_blocked(to_blocked(g, gcb) if gcb else g, gcb, None, 0.0, W, to_blocked(x, xcb) if xcb else x, xcb,
                                                   st_light[:rows], gamma, beta, False, 0.0, 0, None)
            return (from_blocked(r[0], xcb) if xcb else r[0],) + tuple(r[1:])
        return dense.fused_linear_bwd_all(g, None, 0.0, W, x, st_light[:rows], gamma, beta, False, 0.0, 0)

    def heavy(g, x, rows, gcb=0, xcb=0):
        mask = masks[rows]
        if gcb or xcb:
            r = dense.fused_linear_bwd_all_blocked(to_blocked(g, gcb) if gcb else g, gcb, mask, P_OUT, W, to_blocked(x, xcb) if xcb else x, xcb,
                                                   st_heavy[:rows], gamma, beta, True, P_IN, SEED_IN, None)
            return (from_blocked(r[0], xcb) if xcb else r[0],) + tuple(r[1:])
        return dense.fused_linear_bwd_all(g, mask, P_OUT, W, x, st_heavy[:rows], gamma, beta, True, P_IN, SEED_IN)

    # ---- float64 restatement (tests/test_gpu_dense.py), once per kernel kind
    Gd, Wd, xd, gd, bd = G[:n].double(), W.double(), X[:n].double(), gamma.double(), beta.double()

    def reference(kind):
        if kind == "light":
            t, ga, keep = xd, Gd, torch.ones_like(xd)
        else:
            t = torch.relu(xd)
            ga = Gd * (y_N[:n] > 0) / (1.0 - P_OUT)
            # the input dropout's keep mask, from the forward kernel itself: with W = 1 and no epilogue its output IS the dropped u
            u32, _ = dense.fused_linear_fwd(X[:n], torch.eye(D, device=device), None, gamma, beta, EPS, True, P_IN, SEED_IN, False, 0.0, 0)
            keep = (u32 != 0).double() / (1.0 - P_IN)
        mean = t.mean(1, keepdim=True)
        rstd = (((t - mean) ** 2).mean(1, keepdim=True) + EPS).rsqrt()
        xh = (t - mean) * rstd
        u = (xh * gd + bd) * keep
        gu = (ga @ Wd) * keep
        return ga.t() @ u, ga.sum(0), (gu * xh).sum(0), gu.sum(0)

    layouts = [("row-major", lambda t: t, 0, 0), ("ld=160", wide, 0, 0)]
    layouts += [(f"gy blocked by {cb}", lambda t: t, cb, 0) for cb in BLOCKS] + [(f"x and gx blocked by {cb}", lambda t: t, 0, cb) for cb in BLOCKS]
    for kind, fn in (("light", light), ("heavy", heavy)):
        ref_gw, ref_gb, ref_dg, ref_db = reference(kind)
        for name, view, gcb, xcb in layouts:
            gx_n, dg, db, gw, gb = fn(view(G[:n]), view(X[:n]), n, gcb, xcb)
            for N in larger:
                gx_N = fn(view(G[:N]), view(X[:N]), N, gcb, xcb)[0]
                same(gx_n, gx_N[:n], f"{kind} backward, {name}, {n} of {N} rows: gx")
            what = f"{kind} backward, {name}, n = {n}"
            close(gw.double(), ref_gw, what + ": gW")
            close(gb.double(), ref_gb, what + ": gb")
            close(dg.double(), ref_dg, what + ": dgamma")
            close(db.double(), ref_db, what + ": dbeta")

    # the plain Linear with a second gradient branch summed in (acc_in), row-major and ld = 160
    for name, view in (("row-major", lambda t: t), ("ld=160", wide)):
        A = torch.randn(max(larger), D, generator=gen).to(device)
        gx_n = dense.fused_linear_bwd_all(view(G[:n]), None, 0.0, W, view(X[:n]), None, None, None, False, 0.0, 0, acc_in=view(A[:n].clone()))[0]
        for N in larger:
            gx_N = dense.fused_linear_bwd_all(view(G[:N]), None, 0.0, W, view(X[:N]), None, None, None, False, 0.0, 0, acc_in=view(A[:N].clone()))[0]
            same(gx_n, gx_N[:n], f"plain backward with acc_in, {name}, {n} of {N} rows: gx")
