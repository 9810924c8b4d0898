"""GPU: exclude-self Deep Sets aggregation without the k^2 expansion (csrc/loo.hip) against float64 evaluations and
against the expansion path (``preprocessing.expand_edge_index`` + the ordinary ``deepsets_aggregate`` / ``SetGNN``).

Error model used throughout: an fp32 sum of n terms, in any order, is within (n - 1) * 2^-24 * sum |term| of the exact sum (first
order); every scale factor applied to a term or to the sum adds one rounding (2^-24 relative).  The bounds below are
``n * 2^-23 * sum |terms actually summed|`` -- twice the first-order worst case, which leaves room for the scale roundings -- and are
relative to the k - 1 terms an output stands for, never to the segment's total."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import util

pytestmark = pytest.mark.gpu

U = 2.0 ** -23

# Segment sizes of the sweep: 0, 1, 2, 3, 63, 64, 65, 257, 1025 and one size on each side of every boundary of csrc/loo.hip:
#   rows a wave holds in registers (NS * kLooRows = 512 / d... ): 64 (d = 4), 32 (d = 64), 16 (d = 128), 8 (d = 256, 512)
#   wave kernel | workgroup kernel (kLooLong):                     64
#   rows a workgroup holds in registers (8 waves):                 512 (d = 4), 256 (d = 64), 128 (d = 128), 64 (d = 256, 512)
#   tile of the two-sweep path (kLooRows = 8 rows per lane group): sizes that leave runs of 8 k and 8 k +- 1 rows are among the above
SIZES = [0, 1, 2, 3, 7, 8, 9, 15, 16, 17, 0, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, 1, 0]
WIDTHS = [4, 64, 128, 256, 512]


def _segments(sizes, device):
    rowptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(sizes), 0)
    return rowptr.to(torch.int32).to(device), int(rowptr[-1])


def _loo64(rows64, sizes):
    """Float64 "sum of all other rows" per segment as exclusive prefix + exclusive suffix (no subtraction), and the same over |rows|."""
    out, mag = torch.zeros_like(rows64), torch.zeros_like(rows64)
    at = 0
    for k in sizes:
        seg = rows64[at:at + k]
        if k == 1:
            out[at], mag[at] = seg[0], seg[0].abs()
        elif k > 1:
            for src, dst in ((seg, out), (seg.abs(), mag)):
                inc = torch.cumsum(src, 0)
                rinc = torch.flip(torch.cumsum(torch.flip(src, [0]), 0), [0])
                dst[at:at + k] = torch.cat([torch.zeros_like(src[:1]), inc[:-1]]) + torch.cat([rinc[1:], torch.zeros_like(src[:1])])
        at += k
    return out, mag


def _check_loo(ops, device, d, sizes, gathered, scaled, long_mode, seed, table=None):
    g = torch.Generator().manual_seed(seed)
    rowptr, nnz = _segments(sizes, device)
    n_src = 300 if gathered else nnz
    src = (torch.randn(n_src, d, generator=g) if table is None else table).to(device)
    col = torch.randint(0, n_src, (nnz,), generator=g).to(torch.int32).to(device) if gathered else None
    s_src = (0.5 + 1.5 * torch.rand(n_src, generator=g)).to(device) if scaled else None
    s_seg = (0.5 + 1.5 * torch.rand(len(sizes), generator=g)).to(device) if scaled else None
    kw = {}
    if long_mode == "list":
        kw["long_seg"] = torch.tensor([i for i, k in enumerate(sizes) if k > ops.loo_long_threshold()], dtype=torch.int32, device=device)
    elif long_mode == "none":
        kw["n_long"] = 0                                   # "there is no long segment": one wave takes each, however long
    got = ops.loo_rows(rowptr, col, src, s_src, s_seg, **kw)
    assert got.shape == (nnz, d) and got.dtype == torch.float32
    rows = src.double() if col is None else src.double()[col.long()]
    if s_src is not None:
        rows = rows * (s_src.double() if col is None else s_src.double()[col.long()]).unsqueeze(1)
    ref, mag = _loo64(rows, sizes)
    kk = torch.repeat_interleave(torch.tensor(sizes), torch.tensor(sizes)).to(device).double().unsqueeze(1)
    if s_seg is not None:
        seg = torch.repeat_interleave(s_seg.double(), torch.tensor(sizes, device=device)).unsqueeze(1)
        ref, mag = ref * seg, mag * seg
    err = (got.double() - ref).abs()
    bound = kk * U * mag
    worst = float((err / bound.clamp_min(1e-300)).max()) if nnz else 0.0
    print(f"loo_rows d={d} gathered={gathered} scaled={scaled} long={long_mode}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"max err / bound = {worst}"


# ---- (a) the sweep --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scaled", [False, True])
@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("d", WIDTHS)
def test_loo_rows_sweep(device, d, gathered, scaled):
    from allset_amd import ops
    assert ops.loo_long_threshold() == 64                 # the boundaries SIZES was written for
    _check_loo(ops, device, d, SIZES, gathered, scaled, "list", seed=d + 2 * gathered + scaled)


@pytest.mark.parametrize("long_mode", ["scan", "none"])
@pytest.mark.parametrize("d", [64, 128, 512])
def test_loo_rows_without_a_long_list(device, d, long_mode):
    """The same sums when the caller does not list the long segments (every workgroup looks) or states there are none (one wave each)."""
    from allset_amd import ops
    _check_loo(ops, device, d, SIZES, True, True, long_mode, seed=7 + d)


# ---- (b) a row of magnitude 1e6 among O(1) rows ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("gathered", [True, False])
def test_loo_rows_hostile_row(device, gathered):
    """k = 8, one member of magnitude 1e6: the seven outputs that include it are ~1e6, the one that omits it is O(1) and must be exact
    to 8 * 2^-23 of ITS terms (~3e-6) -- "total minus own row" leaves ~1e6 * 2^-24 = 0.06 there."""
    from allset_amd import ops
    g = torch.Generator().manual_seed(11)
    sizes = [8] * 6
    n = 300 if gathered else sum(sizes)
    table = torch.randn(n, 128, generator=g)
    table[::5] *= 1.0e6                                     # gathered: a fifth of the table; contiguous: rows 0, 5, 10, ...
    _check_loo(ops, device, 128, sizes, gathered, True, "list", seed=12, table=table)


# ---- (c) functional parity against the expansion ----------------------------------------------------------------------------------------
def _hypergraph(name):
    """V->E edge list (hyperedge ids from n_v), sorted by vertex.  'small': 50 vertices, 20 hyperedges of sizes 1..9 (two singletons, the
    last vertex isolated); 'long': one hyperedge of 1025 members among 1100 vertices plus 12 small ones."""
    rng = np.random.default_rng(3)
    if name == "small":
        n_v, sizes = 50, [1, 1] + [int(k) for k in rng.integers(2, 10, size=18)]
    else:
        n_v, sizes = 1100, [1025] + [int(k) for k in rng.integers(1, 7, size=12)]
    pairs = []
    for e, k in enumerate(sizes):
        pairs += [(int(v), e + n_v) for v in rng.choice(n_v - 1, size=k, replace=False)]
    return n_v, len(sizes), torch.tensor(sorted(pairs), dtype=torch.int64).t().contiguous()


def _expanded(n_v, n_e, ei, normtype):
    from allset_amd import preprocessing as P
    data = SimpleNamespace(edge_index=ei.clone(), n_x=[n_v], num_hyperedges=[n_e])
    data = P.norm_contruction(P.expand_edge_index(data), option=normtype)
    return data.edge_index, data.norm


@pytest.fixture(scope="module")
def functional_refs(device):
    """Per (graph, aggr, normtype): the expanded list, its float64 weights as dense matrices (V->E: [rows, n_v]; E->V: its transpose
    pattern with the E->V weights), computed once."""
    out = {}
    for graph in ("small", "long"):
        n_v, n_e, ei = _hypergraph(graph)
        for normtype in ("all_one", "deg_half_sym"):
            eie, norm = _expanded(n_v, n_e, ei, normtype)
            ev, ep = eie[0], eie[1] - n_v
            n_rows, n_dst = int(ep.max()) + 1, int(ev.max()) + 1
            size, deg = torch.bincount(ep).double(), torch.bincount(ev, minlength=n_v).double()
            w = torch.ones(ev.numel(), dtype=torch.float64) if normtype == "all_one" else deg[ev].pow(-0.5) * size[ep].pow(-0.5)
            for aggr in ("add", "mean"):
                A = torch.zeros(n_rows, n_v, dtype=torch.float64)
                A[ep, ev] = w / size[ep] if aggr == "mean" else w
                B = torch.zeros(n_dst, n_rows, dtype=torch.float64)
                B[ev, ep] = w / deg[ev] if aggr == "mean" else w
                out[graph, aggr, normtype] = dict(n_v=n_v, ei=ei, eie=eie, norm=norm, A=A.to(device), B=B.to(device),
                                                  size=size.to(device), deg=deg.to(device), ev=ev.to(device), ep=ep.to(device))
    return out


@pytest.mark.parametrize("normtype", ["all_one", "deg_half_sym"])
@pytest.mark.parametrize("aggr", ["add", "mean"])
@pytest.mark.parametrize("graph", ["small", "long"])
def test_functional_parity_with_the_expansion(device, functional_refs, graph, aggr, normtype):
    """Both directions, forward and input gradient, new path and expansion path, each against the float64 product with the dense
    expanded incidence.  Bound per output: (terms + 8) * 2^-23 * (|M| @ |input|), with `terms` the number of products an output sums --
    V->E forward / E->V backward: the expanded hyperedge's size; E->V forward / V->E backward: the expanded degree of the vertex, plus
    the largest expanded hyperedge size among its hyperedges for the new path's first stage (bound (a) of the first stage carried
    through the second stage's sum) -- and 8 for the roundings of the scale factors (pow(-1/2), reciprocals and their products)."""
    from allset_amd import Incidence, LeaveOneOutIncidence, deepsets_aggregate, deepsets_aggregate_exclude_self
    r = functional_refs[graph, aggr, normtype]
    n_v, d = r["n_v"], 64
    g = torch.Generator().manual_seed(5)
    eie = r["eie"].clone().to(device)
    eie[1] -= n_v
    inc = Incidence.from_edge_index(eie, n_src=n_v)
    norm = r["norm"].to(device)
    loo = LeaveOneOutIncidence(r["ei"].to(device), n_v=n_v, e_base=n_v)
    A, B = r["A"], r["B"]
    assert loo.nnz == A.shape[0] == inc.n_dst and loo.n_dst == B.shape[0] == inc.reversed().n_dst
    size_of_row = r["size"]                                              # bincount over the expanded hyperedge ids
    kmax_of_v = torch.zeros(n_v, dtype=torch.float64, device=device).index_reduce_(0, r["ev"], r["size"][r["ep"]], "amax")
    terms_e = size_of_row.unsqueeze(1)                                   # per expanded hyperedge
    terms_v = (r["deg"] + kmax_of_v).unsqueeze(1)                        # per vertex

    def check(what, got, M, inp, terms):
        ref = M @ inp.double()
        bound = (terms[:ref.shape[0]] + 8) * U * (M.abs() @ inp.double().abs())
        err = (got.double() - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"{graph} {aggr} {normtype} {what}: max err / bound = {worst:.3f}")
        assert got.shape == ref.shape and bool((err <= bound).all()), f"{what}: max err / bound = {worst}"

    x = torch.randn(n_v, d, generator=g).to(device)
    y = torch.randn(A.shape[0], d, generator=g).to(device)
    G_e = torch.randn(A.shape[0], d, generator=g).to(device)
    G_v = torch.randn(B.shape[0], d, generator=g).to(device)
    for name, fn_v2e, fn_e2v in (
            ("loo", lambda t: deepsets_aggregate_exclude_self(t, loo, "v2e", aggr, normtype),
             lambda t: deepsets_aggregate_exclude_self(t, loo, "e2v", aggr, normtype)),
            ("expansion", lambda t: deepsets_aggregate(t, inc, norm, aggr), lambda t: deepsets_aggregate(t, inc.reversed(), norm, aggr))):
        xv = x.clone().requires_grad_(True)
        out = fn_v2e(xv)
        (gx,) = torch.autograd.grad(out, xv, G_e)
        check(f"{name} v2e forward", out.detach(), A, x, terms_e)
        check(f"{name} v2e input gradient", gx, A.t(), G_e, terms_v)
        yv = y.clone().requires_grad_(True)
        out = fn_e2v(yv)
        (gy,) = torch.autograd.grad(out, yv, G_v)
        check(f"{name} e2v forward", out.detach(), B, y, terms_v)
        check(f"{name} e2v input gradient", gy, B.t(), G_v, terms_e)


# ---- (d) model parity --------------------------------------------------------------------------------------------------------------------
def _run_model(args, sd, data, device, name):
    """SetGNN forward + backward of (logits * G).sum() in eval mode; the result dict of util.run_product."""
    from allset_amd import SetGNN
    model = SetGNN(args)
    model.load_state_dict(sd)
    model.eval().to(device)
    grabbed = {}
    model.V2EConvs[0].register_forward_hook(lambda m, i, o: grabbed.__setitem__("v2e0", o))
    model.E2VConvs[0].register_forward_hook(lambda m, i, o: grabbed.__setitem__("e2v0", o))
    logits = model(data)
    G = torch.from_numpy(cases.cotangent(name, logits.shape)).to(device)
    (logits * G).sum().backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().cpu() for k, p in model.named_parameters()}
    return dict(logits=logits.detach().cpu(), v2e0=grabbed["v2e0"].detach().cpu(), e2v0=grabbed["e2v0"].detach().cpu(),
                grad_x=data.x.grad.detach().cpu(), grads=grads, model=model)


def _model_pair(device, layers, normtype="all_one"):
    from allset_amd import SetGNN
    from allset_amd import preprocessing as P
    n_v, n_e, ei = _hypergraph("small")
    F, hidden, C = 24, 64, 5
    args = cases.make_args("ds_add", F, hidden, C, All_num_layers=layers)
    spec = [(k, tuple(v.shape)) for k, v in SetGNN(args).state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in cases.make_state_dict(spec, 17 + layers, kinkfree=True).items()}
    x = torch.from_numpy(np.random.default_rng(layers).standard_normal((n_v, F)).astype(np.float32))
    eie, norm = _expanded(n_v, n_e, ei, normtype)
    expanded = SimpleNamespace(x=x.clone().to(device).requires_grad_(True), edge_index=eie.to(device), norm=norm.to(device))
    plain = P.exclude_self(SimpleNamespace(x=x.clone().to(device).requires_grad_(True), edge_index=ei.clone().to(device),
                                           n_x=[n_v], num_hyperedges=[n_e]), normtype=normtype)
    return args, sd, plain, expanded


@pytest.mark.parametrize("normtype", ["all_one", "deg_half_sym"])
@pytest.mark.parametrize("layers", [1, 2])
def test_model_parity_with_the_expanded_model(device, layers, normtype):
    """The same state_dict on unexpanded exclude-self data and on the expanded data: logits, the first layer's conv outputs, the input
    gradient and EVERY parameter gradient, with the helper and tolerance of the SetGNN parity tests (tests/test_gpu_parity.py: fp32,
    rtol = atol = 1e-4 of each tensor's scale).  kinkfree biases: two fp32 evaluations agree on every relu's side."""
    args, sd, plain, expanded = _model_pair(device, layers, normtype)
    want = _run_model(args, sd, expanded, device, f"loo_L{layers}")
    got = _run_model(args, sd, plain, device, f"loo_L{layers}")
    assert list(got["model"].state_dict()) == list(want["model"].state_dict())
    g = {"out_" + k: want[k].numpy() for k in ("logits", "v2e0", "e2v0", "grad_x")}
    g.update({"n_rows_" + k: np.int64(want[k].shape[0]) for k in ("logits", "v2e0", "e2v0")})
    g.update({"grad_" + k: v.numpy() for k, v in want["grads"].items()})
    assert got["v2e0"].shape[0] == plain.edge_index.shape[1]          # hyperedge-side activations: one row per incidence
    assert any(float(v.abs().max()) > 0 for v in want["grads"].values())
    util.assert_matches_golden(got, g, False, rtol=1e-4, atol=1e-4)


def test_graphed_train_step_equals_eager(device):
    """The new path captures (nothing in it synchronises): three replayed steps equal three eager steps."""
    from allset_amd import SetGNN, dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    args, sd, plain, _ = _model_pair(device, 2, "deg_half_sym")
    plain.x = plain.x.detach()
    model = SetGNN(args)
    model.load_state_dict(sd)
    model.to(device)
    n_out = int(plain.edge_index[0].max()) + 1            # the reference's sizing rule: the last vertex has no incidence, so no logits row
    y = torch.randint(0, args.num_classes, (n_out,), generator=torch.Generator().manual_seed(1)).to(device)
    loss_fn = lambda out: torch.nn.functional.cross_entropy(out, y)
    eager = copy.deepcopy(model)
    opt_e = FusedAdam(eager.parameters(), lr=0.01)
    eager.eval()
    for _ in range(3):
        opt_e.zero_grad()
        with dense.deferred_param_grads():
            loss_fn(eager(plain)).backward()
        opt_e.step()
    step = GraphedTrainStep(model, plain, loss_fn, FusedAdam(model.parameters(), lr=0.01), train_mode=False)
    for _ in range(3):
        step()
    torch.cuda.synchronize()
    for (k, a), (_, b) in zip(model.named_parameters(), eager.named_parameters()):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-5, msg=lambda m, k=k: f"{k}: {m}")


# ---- (e) refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals(device):
    from allset_amd import LeaveOneOutIncidence, SetGNN, _lib, deepsets_aggregate_exclude_self, ops
    from allset_amd import preprocessing as P
    n_v, n_e, ei = _hypergraph("small")
    loo = LeaveOneOutIncidence(ei.to(device), n_v=n_v, e_base=n_v)
    x = torch.randn(n_v, 64, device=device)
    for aggr in ("max", "min"):
        with pytest.raises(NotImplementedError, match="expand"):
            deepsets_aggregate_exclude_self(x, loo, "v2e", aggr)
    with pytest.raises(NotImplementedError, match="expand"):
        deepsets_aggregate_exclude_self(x.bfloat16(), loo, "v2e", "add")
    with pytest.raises(NotImplementedError):
        deepsets_aggregate_exclude_self(x, loo, "v2e", "add", "other_norm")
    with pytest.raises(ValueError):
        deepsets_aggregate_exclude_self(x, loo, "sideways")
    with pytest.raises(ValueError):
        deepsets_aggregate_exclude_self(x, loo, "e2v")                 # E->V takes one row per incidence
    with pytest.raises(_lib.AllSetHipError, match="not built"):
        ops.loo_rows(loo.e_rowptr, loo.e_col, torch.randn(n_v, 6, device=device))
    with pytest.raises(_lib.AllSetHipError, match="not built"):
        ops.loo_rows(loo.e_rowptr, loo.e_col, torch.randn(n_v, 516, device=device))
    with pytest.raises(_lib.AllSetHipError):
        ops.loo_rows(loo.e_rowptr, loo.e_col, x.cpu())                 # no CPU fallback
    data = P.exclude_self(SimpleNamespace(x=torch.randn(n_v, 24, device=device), edge_index=ei.clone().to(device), n_x=[n_v],
                                          num_hyperedges=[n_e]))
    pma = SetGNN(cases.make_args("pma_h1", 24, 64, 5)).to(device).eval()
    with pytest.raises(NotImplementedError, match="PMA"):
        pma(data)
    margs = cases.make_args("ds_add", 24, 64, 5, LearnMask=True)
    masked = SetGNN(margs, norm=torch.ones(ei.shape[1])).to(device).eval()
    with pytest.raises(NotImplementedError, match="LearnMask"):
        masked(data)
