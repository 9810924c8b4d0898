"""GPU: CEGCN without the materialised clique expansion (csrc/scan.hip) -- the segmented exclusive scan against
float64, ``functional.clique_propagate`` against the explicit path and float64, the model on ``ConstructV2V_implicit`` data against the
REFERENCE's recorded results (tests/golden/baselines_ce*.npz), capture, the driver flag, and the memory bound.

Error model of the scan tests: an fp32 sum of m terms, in any order, is within (m - 1) * 2^-24 * sum |term| of the exact sum (first
order); the scale applied to each term adds one rounding.  The bound is ``m * 2^-23 * sum |terms the output names|`` -- twice the
first-order worst case -- taken in float64, relative to the terms an output names and never to the segment's total."""
import copy
import ctypes
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ce_cases as cc  # noqa: E402
import ce_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = torch.device("cuda:0")
TOL = dict(rtol=1e-4, atol=1e-4)
U = 2.0 ** -23

# 0, 1, 2; the rows a lane group holds in registers (8 | 9); two runs (16 | 17); the wave kernel's last size and the workgroup
# kernel's first (allset_loo_long_threshold() = 64 | 65); 129; 1025 (two-sweep runs in the workgroup kernel at every width)
SIZES = [0, 1, 2, 8, 9, 16, 17, 64, 65, 129, 1025, 1, 0]
WIDTHS = [4, 12, 64, 128, 256, 260, 512]


def _segments(sizes):
    rowptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(sizes), 0)
    return rowptr.to(torch.int32).to(DEV), int(rowptr[-1])


def _scan64(rows, sizes, reverse):
    """Float64 exclusive prefix (suffix) per segment of ``rows`` and of ``|rows|``, and the number of terms of every output."""
    out, mag = torch.zeros_like(rows), torch.zeros_like(rows)
    terms = torch.zeros(rows.shape[0], dtype=torch.float64, device=rows.device)
    at = 0
    for k in sizes:
        if k > 1:
            for src, dst in ((rows[at:at + k], out), (rows[at:at + k].abs(), mag)):
                if reverse:
                    dst[at:at + k - 1] = torch.flip(torch.cumsum(torch.flip(src[1:], [0]), 0), [0])
                else:
                    dst[at + 1:at + k] = torch.cumsum(src[:-1], 0)
        r = torch.arange(k, dtype=torch.float64, device=rows.device)
        terms[at:at + k] = (k - 1 - r) if reverse else r
        at += k
    return out, mag, terms.unsqueeze(1)


def _check_scan(d, sizes, reverse, gathered, scaled, long_mode, seed, table=None):
    from allset_amd import ops
    g = torch.Generator().manual_seed(seed)
    rowptr, nnz = _segments(sizes)
    n_src = 300 if gathered else nnz
    src = (torch.randn(n_src, d, generator=g) if table is None else table).to(DEV)
    col = torch.randint(0, n_src, (nnz,), generator=g).to(torch.int32).to(DEV) if gathered else None
    s_src = (0.5 + 1.5 * torch.rand(n_src, generator=g)).to(DEV) if scaled else None
    kw = {}
    if long_mode == "list":
        kw["long_seg"] = torch.tensor([i for i, k in enumerate(sizes) if k > ops.loo_long_threshold()], dtype=torch.int32, device=DEV)
    elif long_mode == "none":
        kw["n_long"] = 0                                   # "there is no long segment": one wave takes each, however long
    got = ops.scan_rows(rowptr, col, src, s_src, reverse=reverse, **kw)
    assert got.shape == (nnz, d) and got.dtype == torch.float32
    rows = src.double() if col is None else src.double()[col.long()]
    if s_src is not None:
        rows = rows * (s_src.double() if col is None else s_src.double()[col.long()]).unsqueeze(1)
    ref, mag, terms = _scan64(rows, sizes, reverse)
    err = (got.double() - ref).abs()
    bound = terms * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max()) if nnz else 0.0
    print(f"scan_rows d={d} reverse={reverse} gathered={gathered} scaled={scaled} long={long_mode}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"max err / bound = {worst}"
    none = (terms == 0).expand_as(got)
    assert bool(none.any()) and bool((got[none] == 0).all())          # an output that names no term is exactly 0


# ---- 1. ops.scan_rows ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("d", WIDTHS)
def test_scan_rows_sweep(d, reverse, gathered):
    from allset_amd import ops
    assert ops.loo_long_threshold() == 64                 # the boundaries SIZES was written for
    for scaled in (True, False):
        for long_mode in ("list", "none", "scan"):        # long_seg given, n_long = 0, n_long < 0
            _check_scan(d, SIZES, reverse, gathered, scaled, long_mode, seed=d + 2 * gathered + scaled)


@pytest.mark.parametrize("reverse", [False, True])
def test_scan_rows_4096_row_segment(reverse):
    _check_scan(128, [3, 4096, 0, 5], reverse, True, True, "list", seed=21)
    _check_scan(128, [3, 4096, 0, 5], reverse, False, False, "scan", seed=22)


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("reverse", [False, True])
def test_scan_rows_hostile_row(reverse, gathered):
    """Segments of 8 rows of O(1) with one member of magnitude 1e6 -- LAST in its segment for the prefix, FIRST for the suffix, so no
    output of its segment names it: all of them must meet the bound of their own O(1) terms (~8 * 2^-23 * 8), which a "total minus
    the rest" could not (1e6 * 2^-24 = 0.06).  A second set of segments has it in the middle: outputs before it stay O(1)-accurate."""
    g = torch.Generator().manual_seed(11)
    sizes = [8] * 8
    nnz = sum(sizes)
    rows = torch.randn(nnz, 128, generator=g)
    big = [(7 if not reverse else 0) + 8 * s for s in range(4)] + [3 + 8 * s for s in range(4, 8)]
    rows[big] *= 1.0e6
    if gathered:                                           # the same rows through a permutation
        perm = torch.randperm(nnz, generator=g)
        table = torch.empty_like(rows)
        table[perm] = rows
        from allset_amd import ops
        rowptr, _ = _segments(sizes)
        got = ops.scan_rows(rowptr, perm.to(torch.int32).to(DEV), table.to(DEV), None, reverse=reverse)
    else:
        from allset_amd import ops
        rowptr, _ = _segments(sizes)
        got = ops.scan_rows(rowptr, None, rows.to(DEV), None, reverse=reverse)
    ref, mag, terms = _scan64(rows.double().to(DEV), sizes, reverse)
    err = (got.double() - ref).abs()
    bound = terms * U * mag
    assert bool((err <= bound).all()), f"max err / bound = {float((err / bound.clamp_min(1e-300)).max())}"
    clean = mag < 1e3                                                  # the outputs that do not name a 1e6 row
    assert int(clean.sum()) >= (4 * 8 + 4 * 4) * 128                   # all of the first four segments, four or five of each other one
    assert float(err[clean].max()) < 8 * U * 8 * 6.0                   # O(1) accurate in absolute terms too (|N(0,1)| < 6)


def test_scan_rows_argument_validation():
    """Status code + message, and nothing is launched: the output buffer keeps its sentinel."""
    from allset_amd import _lib
    lib = _lib.load()
    sizes = [3, 5]
    rowptr, nnz = _segments(sizes)
    d = 8
    buf = torch.randn(nnz * d + 4, device=DEV)
    src = buf[:nnz * d].view(nnz, d)
    out = torch.full((nnz, d), -7.0, device=DEV)
    P = ctypes.c_void_p
    stream = torch.cuda.current_stream().cuda_stream

    def call(src_ptr, out_ptr, lds, ldo, n_long, dd, long_ptr=None):
        return lib.allset_scan_rows(P(rowptr.data_ptr()), None, P(src_ptr), lds, None, P(out_ptr), ldo, long_ptr, n_long, 0, len(sizes),
                                    nnz, nnz, dd, stream)

    def refused(rc, code, word):
        msg = lib.allset_last_error().decode()
        assert rc == code and "scan_rows" in msg and word in msg, (rc, msg)

    refused(call(src.data_ptr() + 4, out.data_ptr(), d, d, 0, d), -1, "aligned")          # misaligned rows
    refused(call(src.data_ptr(), out.data_ptr() + 8, d, d, 0, d), -1, "aligned")
    refused(call(src.data_ptr(), out.data_ptr(), d + 2, d, 0, d), -1, "aligned")          # a leading dimension that is no multiple of 4
    refused(call(src.data_ptr(), out.data_ptr(), 8, 8, 0, 6), -3, "not built")            # d % 4 != 0
    refused(call(src.data_ptr(), out.data_ptr(), 516, 516, 0, 516), -3, "not built")      # d > 512
    refused(call(src.data_ptr(), src.data_ptr(), d, d, 0, d), -1, "alias")                # out aliasing src
    long_seg = torch.zeros(4, dtype=torch.int32, device=DEV)
    refused(call(src.data_ptr(), out.data_ptr(), d, d, 3, d, P(long_seg.data_ptr())), -1, "n_long")   # n_long > n_seg
    refused(call(src.data_ptr(), out.data_ptr(), d, d, 1, d, None), -1, "long_seg")       # a count without the list
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert call(src.data_ptr(), out.data_ptr(), d, d, 0, d) == 0                          # and the good call runs
    torch.cuda.synchronize()
    assert bool((out[0] == 0).all()) and bool((out[1] == src[0]).all())


# ---- 2. clique_propagate against the explicit path and float64 ----------------------------------------------------------------------
N_V, INTERIOR, TRAILING = 1400, (11, 12), 4


def _hypergraph():
    """(vertex, hyperedge) incidences over 1400 vertices: 120 hyperedges of sizes 1..8 (a few of one member) and one of 70 members among
    the first 296 vertices, one of 1100 members (which needs that many vertices) over all of them, a pair shared by three more
    hyperedges, vertices 11 and 12 and the last 4 in no hyperedge; one incidence is listed twice."""
    rng = np.random.default_rng(5)
    low = np.array([v for v in range(296) if v not in INTERIOR])
    pool = np.array([v for v in range(N_V - TRAILING) if v not in INTERIOR])
    pairs = set()
    for e in range(120):
        k = 1 if e % 17 == 3 else int(rng.integers(2, 9))
        pairs |= {(int(v), e) for v in rng.choice(low, size=k, replace=False)}
    for e in range(120, 123):
        pairs |= {(int(low[0]), e), (int(low[1]), e)}
    pairs |= {(int(v), 123) for v in rng.choice(low, size=70, replace=False)}
    pairs |= {(int(v), 124) for v in rng.choice(pool, size=1100, replace=False)}
    pairs = sorted(pairs)
    ei = torch.tensor(pairs + pairs[:1], dtype=torch.int64).t().contiguous()
    return torch.stack([ei[0], ei[1] + N_V])              # hyperedge ids behind the vertex ids, as ExtractV2E leaves them


@pytest.fixture(scope="module")
def graphs():
    """Once: the explicit graph, the implicit graph, and the float64 normalised adjacency ``M`` (``y = M @ x``) of the restatement
    (tests/ce_oracle.py ``clique_expansion`` + ``gcn_norm``, as a dense [n, n] matrix so that C = 512 costs one matmul)."""
    from allset_amd.baselines import CEGraph, ImplicitCEGraph
    from allset_amd.preprocessing import ConstructV2V, ConstructV2V_implicit, norm_contruction
    ei = _hypergraph()
    ex = norm_contruction(ConstructV2V(SimpleNamespace(edge_index=ei.clone().to(DEV))), TYPE='V2V')
    explicit = CEGraph(ex.edge_index, ex.norm, N_V)
    im = ConstructV2V_implicit(SimpleNamespace(edge_index=ei.clone().to(DEV)))
    assert im.edge_index.shape[1] == ei.shape[1] - 1      # the duplicate counts once
    implicit = ImplicitCEGraph(im.edge_index, N_V)
    pairs, mult = orc.clique_expansion(ei)
    assert float(mult.max()) >= 3.0
    oei, ow = orc.gcn_norm(pairs, mult)
    M = torch.zeros(N_V, N_V, dtype=torch.float64).index_put_((oei[1], oei[0]), ow, accumulate=True)
    n = int(pairs.max()) + 1
    assert implicit.N == n <= N_V - TRAILING and implicit.n_long == 2 and implicit.dinv.dtype == torch.float32
    assert bool((implicit.deg[list(INTERIOR)] == 1).all()) and bool((implicit.deg[n:] == 0).all())
    return dict(explicit=explicit, implicit=implicit, M=M, n=n)


@pytest.mark.parametrize("act,p", [(None, 0.0), ("relu", 0.5)])
@pytest.mark.parametrize("C", [1, 3, 7, 64, 128, 512])
def test_clique_propagate_vs_explicit_and_float64(monkeypatch, graphs, C, act, p):
    """Forward, grad x and grad bias of both paths against float64, at the tolerances of test_weighted_propagate_vs_float64 (rtol = 1e-4,
    atol = 1e-4 * max(1, max |reference|)).  With dropout the restatement gets each product call's own mask.  The cotangent is zero
    where the float64 pre-activation is within 1e-4 of the relu's kink, so that no gradient depends on which side fp32 lands."""
    from allset_amd import dense
    from allset_amd.functional import clique_propagate, weighted_propagate
    M, n = graphs["M"], graphs["n"]
    g = torch.Generator().manual_seed(C)
    x = torch.randn(N_V, C, generator=g, dtype=torch.float64)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    pre = M @ x + b
    G = torch.randn(N_V, C, generator=g, dtype=torch.float64) * ((pre.abs() > 1e-4) if act else 1.0)
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    ex, im = graphs["explicit"], graphs["implicit"]
    for name, fn in (("implicit", lambda t, bb: clique_propagate(t, im, bias=bb, act=act, p=p)),
                     ("explicit", lambda t, bb: weighted_propagate(t, ex.inc, ex.w_dst, ex.w_src, bias=bb, act=act, p=p))):
        del seeds[:]
        xd = x.float().to(DEV).requires_grad_(True)
        bd = b.float().to(DEV).requires_grad_(True)
        y = fn(xd, bd)
        assert y.shape == (N_V, C)
        (y * G.float().to(DEV)).sum().backward()
        mask = dense.dropout_scale((N_V, C), p, seeds[0], DEV).cpu().double() if p > 0 else None
        assert p == 0 or len(seeds) == 1
        xo, bo = x.clone().requires_grad_(True), b.clone().requires_grad_(True)
        yo = M @ xo + bo
        yo = torch.relu(yo) if act == "relu" else yo
        yo = yo * mask if mask is not None else yo
        (yo * G).sum().backward()
        for what, got, want in (("forward", y.detach(), yo.detach()), ("grad x", xd.grad, xo.grad), ("grad bias", bd.grad, bo.grad)):
            scale = max(1.0, float(want.abs().max()))
            err = float((got.cpu().double() - want).abs().max())
            print(f"{name} C={C} act={act} p={p} {what}: max abs err {err:.3e} (atol {1e-4 * scale:.3e})")
            torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=1e-4 * scale, msg=lambda m: f"{name} {what}: {m}")
        if act is None and p == 0:                        # trailing isolated vertices: exactly the bias
            assert torch.equal(y.detach()[n:], bd.detach().expand(N_V - n, C))


def test_clique_propagate_refusals(graphs):
    from allset_amd import _lib
    from allset_amd.functional import clique_propagate
    im = graphs["implicit"]
    with pytest.raises(_lib.AllSetHipError, match="not built"):
        clique_propagate(torch.randn(N_V, 516, device=DEV), im)
    with pytest.raises(NotImplementedError, match="bf16"):
        clique_propagate(torch.randn(N_V, 64, device=DEV).bfloat16(), im)
    with pytest.raises(_lib.AllSetHipError):
        clique_propagate(torch.randn(N_V, 64), im)                      # no CPU fallback
    with pytest.raises(_lib.AllSetHipError):
        clique_propagate(torch.randn(N_V - 1, 64, device=DEV), im)
    with pytest.raises(ValueError):
        clique_propagate(torch.randn(N_V, 64, device=DEV), im, act="gelu")


# ---- 3. the model against the recorded reference ----------------------------------------------------------------------------------------
def _fixture(name):
    return cc.spec(name), cc.load([f for f, ns in cc.FILES.items() if name in ns][0])


def _implicit_case(name):
    from allset_amd.baselines import CEGCN
    from allset_amd.train import HypergraphData, build_model, parse_args, preprocess
    c, fx = _fixture(name)
    x, block, n_v, n_e = cc.raw_data(c)
    args = parse_args(["--method", "CEGCN", "--CE_implicit"])
    data = preprocess(args, HypergraphData(x=torch.from_numpy(x).float(), edge_index=torch.from_numpy(block), n_x=[n_v],
                                           num_hyperedges=[n_e]))
    assert data.clique_implicit and data.norm is None and data.edge_index.device.type == "cpu"
    a = cc.args_of(c)
    torch.manual_seed(c["seed"])
    model = build_model(SimpleNamespace(**{**vars(args), **vars(a)}), data)
    assert isinstance(model, CEGCN)
    model.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in cc.perturb(model.state_dict(), c).items()})
    dd = SimpleNamespace(x=torch.from_numpy(x).float().to(DEV).requires_grad_(True), edge_index=data.edge_index.to(DEV), norm=None,
                         clique_expansion=True, clique_implicit=True)
    return c, fx, model.to(DEV), dd, x


@pytest.mark.parametrize("name", [n for n in sorted(cc.CASES) if not cc.spec(n)["train"]])
def test_implicit_model_equals_recorded_reference(name):
    """Eval-mode cases: logits, grad_x and every parameter gradient against the reference's recorded results, with the helper and the
    tolerances of test_gpu_ce_baselines.py::test_model_equals_recorded_reference."""
    from allset_amd.baselines import ImplicitCEGraph
    c, fx, model, dd, _ = _implicit_case(name)
    model.eval()
    logits = model(dd)
    assert isinstance(model._graph, ImplicitCEGraph)
    G = torch.from_numpy(cc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()

    def scale(key):
        kind, v = cc.result(fx, name, key)
        return max(1.0, float(np.abs(v if kind == "whole" else v[1]).max()))
    cc.assert_result(logits, fx, name, "logits", rtol=1e-4, atol=1e-4 * scale("logits"))
    cc.assert_result(dd.x.grad, fx, name, "grad_x", rtol=1e-4, atol=1e-4 * scale("grad_x"))
    for k, p in model.named_parameters():
        cc.assert_result(p.grad, fx, name, f"grad:{k}", rtol=1e-4, atol=1e-4 * scale(f"grad:{k}"))


@pytest.mark.parametrize("name", [n for n in sorted(cc.CASES) if cc.spec(n)["train"]])
def test_implicit_model_training_mode_with_product_masks(monkeypatch, name):
    """Training-mode cases, as test_gpu_ce_baselines.py handles training mode: the product draws its own hash masks, which are fed to the
    float64 restatement (the restatement against the recorded training-mode results: tests/test_ce_reference.py)."""
    from allset_amd import dense
    c, fx, model, dd, x = _implicit_case(name)
    model.train()
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    logits = model(dd)
    G = torch.from_numpy(cc.cotangent(c, logits.shape[0]))
    (logits * G.float().to(DEV)).sum().backward()
    n_convs = len(model.convs)
    assert len(seeds) == n_convs - 1
    masks = [dense.dropout_scale((c["n_v"], c["hidden"]), cc.DROPOUT, s, DEV).cpu().double() for s in seeds]
    sd = {k: (v.detach().cpu().double().requires_grad_(True) if v.is_floating_point() else v) for k, v in model.state_dict().items()}
    from allset_amd.preprocessing import ExtractV2E
    _, block, n_v, n_e = cc.raw_data(c)
    v2e = ExtractV2E(SimpleNamespace(edge_index=torch.from_numpy(block), n_x=[n_v], num_hyperedges=[n_e])).edge_index
    oei, ow = orc.gcn_norm(*orc.clique_expansion(v2e))
    xo = torch.from_numpy(x).float().double().requires_grad_(True)
    lo = orc.cegcn_forward(sd, xo, oei, ow, n_convs, masks, bn=c["norm"] == "bn", training=True)
    (lo * G).sum().backward()
    torch.testing.assert_close(logits.detach().cpu().double(), lo.detach(), **TOL)
    torch.testing.assert_close(dd.x.grad.cpu().double(), xo.grad, rtol=1e-4, atol=1e-4 * max(1.0, float(xo.grad.abs().max())))
    for k, prm in model.named_parameters():
        torch.testing.assert_close(prm.grad.cpu().double(), sd[k].grad, rtol=1e-4, atol=1e-3, msg=lambda m, k=k: f"{k}: {m}")


# ---- 4. capture and the driver ------------------------------------------------------------------------------------------------------------
def _small_hyperedges(seed, n_v=300, n_e=120, trailing=4, interior=(11, 12)):
    """(vertex, hyperedge) incidences: sizes 1..8 (a few of one member), a pair shared by three more hyperedges, vertices ``interior``
    and the last ``trailing`` in no hyperedge."""
    rng = np.random.default_rng(seed)
    pool = np.array([v for v in range(n_v - trailing) if v not in interior])
    pairs = set()
    for e in range(n_e):
        k = 1 if e % 17 == 3 else int(rng.integers(2, 9))
        pairs |= {(int(v), e) for v in rng.choice(pool, size=k, replace=False)}
    for e in range(n_e, n_e + 3):
        pairs |= {(int(pool[0]), e), (int(pool[1]), e)}
    return torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous(), n_v


def _model_data(L, normalization, seed=0):
    from allset_amd.baselines import CEGCN
    from allset_amd.preprocessing import ConstructV2V_implicit
    ei, n_v = _small_hyperedges(seed)
    data = ConstructV2V_implicit(SimpleNamespace(edge_index=ei))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_v, 24, generator=g)
    torch.manual_seed(seed)
    model = CEGCN(24, 32, 5, L, 0.5, Normalization=normalization)
    for prm in model.parameters():                          # non-zero biases
        with torch.no_grad():
            prm.add_(0.1 * torch.randn(prm.shape, generator=g))
    dd = SimpleNamespace(x=x.to(DEV), edge_index=data.edge_index.to(DEV), norm=None, clique_expansion=True, clique_implicit=True)
    return model.to(DEV), dd, x


@pytest.mark.parametrize("norm", ["ln", "bn"])
def test_graphed_training_mode_step_equals_eager(monkeypatch, norm):
    """The criterion of test_gpu_ce_baselines.py::test_graphed_training_mode_step_equals_eager on implicit data: one replay of the
    captured step equals one eager step that draws its masks from the same device seed counter value and the same per-site salts."""
    from allset_amd import dense
    from allset_amd.baselines import ImplicitCEGraph
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    model, data, x = _model_data(3, norm)
    y = torch.randint(0, 5, (x.shape[0],), device=DEV)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    salts = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: salts.append(real()) or salts[-1])
    step = GraphedTrainStep(model, data, loss_fn, FusedAdam(model.parameters(), lr=0.01), warmup=3)
    assert isinstance(model._graph, ImplicitCEGraph)
    n_sites = len(salts) // 4
    assert n_sites == len(model.convs) - 1
    captured = salts[-n_sites:]
    counter = step.counter.clone()
    loss_g = step().clone()
    torch.cuda.synchronize()
    replay_salts = iter(captured)
    monkeypatch.setattr(dense, "_draw_seed", lambda: next(replay_salts))
    opt = FusedAdam(eager.parameters(), lr=0.01)
    eager.train()
    with dense.device_seed_counter(counter):
        opt.zero_grad()
        loss_e = loss_fn(eager(data))
        loss_e.backward()
    opt.step()
    torch.testing.assert_close(loss_g, loss_e.detach(), rtol=1e-5, atol=1e-6)
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


def test_train_driver_end_to_end(tmp_path):
    cmd = [sys.executable, "-m", "allset_amd.train", "--dname", "synthetic", "--method", "CEGCN", "--CE_implicit", "--epochs", "5",
           "--runs", "1", "--hip_graph", "1", "--res_root", str(tmp_path)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "All done!" in res.stdout and "capture failed" not in res.stdout


def test_driver_refuses_cegat(tmp_path):
    from allset_amd.train import build_model, build_parser
    cmd = [sys.executable, "-m", "allset_amd.train", "--dname", "synthetic", "--method", "CEGAT", "--CE_implicit", "--epochs", "1",
           "--runs", "1", "--res_root", str(tmp_path)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 2 and "--CE_implicit" in res.stderr and "factorise" in res.stderr, res.stderr[-2000:]
    args = build_parser().parse_args(["--method", "CEGAT"])
    args.num_features, args.num_classes = 24, 5
    _, dd, _ = _model_data(2, "ln")
    with pytest.raises(ValueError, match="implicit"):
        build_model(args, dd)


# ---- 5. memory proportional to the incidence ----------------------------------------------------------------------------------------------
def test_memory_is_proportional_to_the_incidence():
    """4200 vertices, one hyperedge of 4096 members plus 50 of size 2..8, C = 16: the expansion would hold 8.39 M pairs.  Graph build +
    forward + backward keep the peak allocation increase under a tenth of 8 B x pairs (the yardstick of the exclude-self memory test);
    the working set is a handful of [~4300, 16] fp32 buffers plus int32 / int64 index vectors.  The explicit path is not run."""
    from allset_amd.baselines import ImplicitCEGraph
    from allset_amd.functional import clique_propagate
    from allset_amd.preprocessing import ConstructV2V_implicit, clique_implicit_structure
    rng = np.random.default_rng(8)
    n_v, C = 4200, 16
    inc = [(int(v), 0) for v in rng.choice(n_v - 10, size=4096, replace=False)]
    for e in range(1, 51):
        inc += [(int(v), e) for v in rng.choice(n_v - 10, size=int(rng.integers(2, 9)), replace=False)]
    ei = torch.tensor(sorted(inc), dtype=torch.int64).t().contiguous()
    ei = torch.stack([ei[0], ei[1] + n_v])
    sizes = torch.bincount(ei[1] - n_v)
    pairs = int((sizes * (sizes - 1) // 2).sum())
    assert pairs > 8_380_000
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n_v, C, generator=g, dtype=torch.float64)
    b = torch.randn(C, generator=g, dtype=torch.float64)
    G = torch.randn(n_v, C, generator=g, dtype=torch.float64)
    ei_d, G_d = ei.to(DEV), G.float().to(DEV)
    xd, bd = x.float().to(DEV).requires_grad_(True), b.float().to(DEV).requires_grad_(True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    data = ConstructV2V_implicit(SimpleNamespace(edge_index=ei_d))
    graph = ImplicitCEGraph(data.edge_index, n_v)
    y = clique_propagate(xd, graph, bias=bd)
    (y * G_d).sum().backward()
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - before
    print(f"peak allocation increase {grew / 1e6:.3f} MB; a tenth of 8 B x {pairs} pairs = {0.8 * pairs / 1e6:.3f} MB")
    assert grew < 0.1 * 8 * pairs
    # the float64 prefix form on the host
    st = clique_implicit_structure(ei, n_v)
    dinv = st["deg"].double().pow(-0.5)
    dinv[torch.isinf(dinv)] = 0

    def prefix_form(t, reverse):
        rows = (dinv.unsqueeze(1) * t)[st["member"]]
        acc = torch.zeros_like(rows)
        ptr = st["e_rowptr"].tolist()
        for a, e in zip(ptr[:-1], ptr[1:]):
            if e - a >= 2:
                if reverse:
                    acc[a:e - 1] = torch.flip(torch.cumsum(torch.flip(rows[a + 1:e], [0]), 0), [0])
                else:
                    acc[a + 1:e] = torch.cumsum(rows[a:e - 1], 0)
        out = torch.zeros_like(t).index_add_(0, st["member"], acc)
        return dinv.unsqueeze(1) * (out + (st["loop"].double() * dinv).unsqueeze(1) * t)
    for what, got, want in (("forward", y.detach(), prefix_form(x, False) + b), ("grad x", xd.grad, prefix_form(G, True)),
                            ("grad bias", bd.grad, G.sum(0))):
        torch.testing.assert_close(got.cpu().double(), want, rtol=1e-4, atol=1e-4 * max(1.0, float(want.abs().max())),
                                   msg=lambda m: f"{what}: {m}")
