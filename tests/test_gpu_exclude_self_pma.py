"""GPU: exclude-self AllSetTransformer without the k^2 expansion -- the leave-one-out softmax of csrc/loo_softmax.hip (DESIGN.md section
20) against float64 evaluations and against the expansion path (``preprocessing.expand_edge_index`` + the ordinary ``pma_aggregate`` /
``SetGNN``).

Tolerance: ``RTOL`` / ``ATOL`` of tests/test_gpu_ops.py (the PMA kernels' own, 1e-4); an error is measured in units of
``ATOL + RTOL * |reference|``.  In the kernel sweep the expansion path runs on the same data against the same float64 values and the new
path's worst error may be at most twice the expansion's (a different summation order), or 1 unit where that is larger."""
import copy
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cases
import util
from test_gpu_exclude_self import SIZES
from test_gpu_ops import ATOL, RTOL

pytestmark = pytest.mark.gpu

SLOPE = 0.2
HEAD_SHAPES = [(1, 4), (1, 64), (4, 32), (8, 16), (4, 64), (8, 64)]


def _units(got, ref):
    """Worst error in units of the tolerance."""
    if ref.numel() == 0:
        return 0.0
    return float(((got.double() - ref).abs() / (ATOL + RTOL * ref.abs())).max())


def _loo_softmax64(a, v, sizes):
    """Float64 leave-one-out softmax per segment, as an explicit loop over j != i: Z_i = sum_{j != i} exp(a_j),
    o_i = sum_{j != i} exp(a_j) v_j / Z_i, L_i = log Z_i; a singleton keeps its row.  a [nnz, H] (activated), v [nnz, H, C]."""
    outs, lses = [], []
    at = 0
    for k in sizes:
        sa, sv = a[at:at + k], v[at:at + k]
        at += k
        if k == 0:
            continue
        if k == 1:
            outs.append(sv)
            lses.append(sa)
            continue
        i = torch.arange(k, device=a.device)
        Z = torch.zeros(k, a.shape[1], dtype=torch.float64, device=a.device)
        N = torch.zeros(k, a.shape[1], v.shape[2], dtype=torch.float64, device=a.device)
        for j in range(k):
            other = (i != j).double().unsqueeze(1)                    # positions i that include member j
            e = torch.exp(sa[j]).unsqueeze(0) * other                 # [k, H]
            Z = Z + e
            N = N + e.unsqueeze(2) * sv[j].unsqueeze(0)
        outs.append(N / Z.unsqueeze(2))
        lses.append(torch.log(Z))
    return torch.cat(outs), torch.cat(lses)


_REFS = {}


def _sweep_case(device, H, C, gathered):
    """Inputs, float64 results and the expansion path's errors for one (H, C, gathered), computed once."""
    key = (H, C, gathered)
    if key in _REFS:
        return _REFS[key]
    from allset_amd import Incidence, pma_aggregate
    from allset_amd import preprocessing as P
    g = torch.Generator().manual_seed(100 * H + C + gathered)
    d, sizes = H * C, SIZES
    rowptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(sizes), 0)
    nnz = int(rowptr[-1])
    n_src = 1100 if gathered else nnz
    V = torch.randn(n_src, d, generator=g).to(device)
    alpha = (1.5 * torch.randn(n_src, H, generator=g)).to(device)
    # members of one segment are distinct rows (the expansion is ill-defined otherwise)
    col = torch.cat([torch.randperm(n_src, generator=g)[:k] for k in sizes]).to(torch.int32).to(device) if gathered else None
    gout = torch.randn(nnz, d, generator=g).to(device)
    glse = torch.randn(nnz, H, generator=g).to(device)
    idx = col.long() if gathered else torch.arange(nnz, device=device)
    V64 = V.double().requires_grad_(True)
    al64 = alpha.double().requires_grad_(True)
    a_pos = torch.nn.functional.leaky_relu(al64, SLOPE)[idx]
    a_pos.retain_grad()
    v_pos = V64[idx].view(nnz, H, C)
    v_pos.retain_grad()
    out64, lse64 = _loo_softmax64(a_pos, v_pos, sizes)
    out64 = out64.reshape(nnz, d)
    loss = (out64 * gout.double()).sum()
    loss.backward(retain_graph=True)                                  # cotangent of out alone: what the expansion path can take
    gV_src_o, ga_src_o = V64.grad.clone(), al64.grad.clone()
    for t in (V64, al64, a_pos, v_pos):
        t.grad = None
    (loss + (lse64 * glse.double()).sum()).backward()
    dact = torch.where(alpha > 0, 1.0, SLOPE).double()[idx]
    ref = dict(out=out64.detach(), lse=lse64.detach(), gV_pos=v_pos.grad.reshape(nnz, d), galpha_pos=a_pos.grad * dact)
    # the expansion path on the same data
    seg = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    ei = torch.stack([idx.cpu(), seg + n_src])
    exp = P.expand_edge_index(SimpleNamespace(edge_index=ei, n_x=[n_src], num_hyperedges=[len(sizes)]))
    eie = exp.edge_index.clone().to(device)
    eie[1] -= n_src
    inc = Incidence.from_edge_index(eie, n_src=n_src, n_dst=nnz)
    Vx, ax = V.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
    o_x, m_x, l_x = pma_aggregate(Vx, ax, inc, H, SLOPE)
    gVx, gax = torch.autograd.grad(o_x, (Vx, ax), gout)
    exp_err = dict(out=_units(o_x.detach(), ref["out"]), lse=_units(m_x + torch.log(l_x), ref["lse"]),
                   gV=_units(gVx, gV_src_o), galpha=_units(gax, ga_src_o))
    hit = _REFS[key] = dict(rowptr=rowptr.to(torch.int32).to(device), col=col, V=V, alpha=alpha, gout=gout, glse=glse, ref=ref,
                            exp_err=exp_err, nnz=nnz, sizes=sizes)
    return hit


# ---- (a) the sweep --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_mode", ["list", "scan", "none"])
@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("H,C", HEAD_SHAPES)
def test_loo_softmax_sweep(device, H, C, gathered, long_mode):
    from allset_amd import ops
    assert ops.loo_long_threshold() == 64                 # the boundaries SIZES was written for
    c = _sweep_case(device, H, C, gathered)
    kw = {}
    if long_mode == "list":
        kw["long_seg"] = torch.tensor([i for i, k in enumerate(c["sizes"]) if k > 64], dtype=torch.int32, device=device)
    elif long_mode == "none":
        kw["n_long"] = 0
    out, lse = ops.loo_softmax_fwd(c["rowptr"], c["col"], c["alpha"], c["V"], H, SLOPE, **kw)
    gV, ga = ops.loo_softmax_bwd(c["rowptr"], c["col"], c["alpha"], c["V"], H, SLOPE, out, lse, c["gout"], c["glse"], **kw)
    assert out.shape == (c["nnz"], H * C) and lse.shape == (c["nnz"], H) and gV.shape == out.shape and ga.shape == lse.shape
    new = {k: _units(t, c["ref"][k]) for k, t in (("out", out), ("lse", lse), ("gV_pos", gV), ("galpha_pos", ga))}
    worst_new, worst_exp = max(new.values()), max(c["exp_err"].values())
    print(f"loo_softmax H={H} C={C} gathered={gathered} long={long_mode}: worst error (tolerance units) new {worst_new:.4f} {new}, "
          f"expansion {worst_exp:.4f} {c['exp_err']}")
    for t in (out, lse, gV, ga):
        assert bool(torch.isfinite(t).all())
    assert worst_new <= max(1.0, 2.0 * worst_exp), (new, c["exp_err"])


# ---- (b) hostile logits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tie", [False, True])
@pytest.mark.parametrize("gathered", [True, False])
def test_hostile_logits(device, gathered, tie):
    """k = 8, one member's logit 100 above the rest (or two such members): the output that omits it is a softmax over the others,
    whose weights are ~exp(-100) of the segment's total -- it must match float64 relative to ITS terms, and so must the gradients.
    Singletons return their row and L = a bit for bit."""
    from allset_amd import ops
    H, C = 4, 32
    g = torch.Generator().manual_seed(21 + tie)
    sizes = [8, 1, 8, 8, 1, 8]
    rowptr = torch.zeros(len(sizes) + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.tensor(sizes), 0)
    nnz = int(rowptr[-1])
    n_src = 64 if gathered else nnz
    col = torch.cat([torch.randperm(n_src, generator=g)[:k] for k in sizes]).to(torch.int32) if gathered else None
    idx = col.long() if gathered else torch.arange(nnz)
    alpha = torch.randn(n_src, H, generator=g)
    for s, k in enumerate(sizes):
        if k == 8:
            at = int(rowptr[s])
            alpha[idx[at + (s % 8)]] += 100.0                         # a different place in each segment (first, third, ...)
            if tie:
                alpha[idx[at + 7 - (s % 4)]] = alpha[idx[at + (s % 8)]]
    V = torch.randn(n_src, H * C, generator=g)
    gout, glse = torch.randn(nnz, H * C, generator=g), torch.randn(nnz, H, generator=g)
    dev = lambda t: t.to(device) if t is not None else None
    rp = rowptr.to(torch.int32).to(device)
    out, lse = ops.loo_softmax_fwd(rp, dev(col), dev(alpha), dev(V), H, SLOPE)
    gV, ga = ops.loo_softmax_bwd(rp, dev(col), dev(alpha), dev(V), H, SLOPE, out, lse, dev(gout), dev(glse))
    a_pos = torch.nn.functional.leaky_relu(alpha.double(), SLOPE)[idx].requires_grad_(True)
    v_pos = V.double()[idx].view(nnz, H, C).requires_grad_(True)
    out64, lse64 = _loo_softmax64(a_pos, v_pos, sizes)
    ((out64.reshape(nnz, -1) * gout.double()).sum() + (lse64 * glse.double()).sum()).backward()
    dact = torch.where(alpha > 0, 1.0, SLOPE).double()[idx]
    ref = dict(out=out64.detach().reshape(nnz, -1), lse=lse64.detach(), gV_pos=v_pos.grad.reshape(nnz, -1), galpha_pos=a_pos.grad * dact)
    got = dict(out=out, lse=lse, gV_pos=gV, galpha_pos=ga)
    for k, t in got.items():
        assert bool(torch.isfinite(t).all()), k
        u = _units(t.cpu(), ref[k])
        print(f"hostile gathered={gathered} tie={tie} {k}: worst error {u:.4f} tolerance units")
        assert u <= 1.0, (k, u)
    for s, k in enumerate(sizes):
        if k == 1:
            p = int(rowptr[s])
            assert torch.equal(out[p].cpu(), V[idx[p]])
            assert torch.equal(lse[p].cpu(), torch.nn.functional.leaky_relu(alpha[idx[p]], SLOPE))


# ---- (c) functional parity against the dense softmax over the expanded incidence -------------------------------------------------------
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


def _expanded(n_v, n_e, ei):
    from allset_amd import preprocessing as P
    data = SimpleNamespace(edge_index=ei.clone(), n_x=[n_v], num_hyperedges=[n_e])
    data = P.norm_contruction(P.expand_edge_index(data), option="all_one")
    return data.edge_index, data.norm


def _dense_pma64(V, alpha, mask, H):
    """Float64 softmax pooling with the dense incidence ``mask`` [targets, sources]."""
    a = torch.nn.functional.leaky_relu(alpha, SLOPE)                                   # [n_s, H]
    has = mask.any(dim=1, keepdim=True)                                                # a target without sources pools to zero
    logits = torch.where((mask | ~has).unsqueeze(2), a.unsqueeze(0), torch.full((), -float("inf"), dtype=torch.float64, device=V.device))
    w = torch.softmax(logits, dim=1) * has.unsqueeze(2)                                # [n_t, n_s, H]
    return torch.einsum("tsh,shc->thc", w, V.view(V.shape[0], H, -1)).reshape(mask.shape[0], -1)


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("graph", ["small", "long"])
def test_functional_parity_with_the_dense_softmax(device, graph, heads):
    """pma_aggregate_exclude_self, both directions, forward and the gradients to V and alpha, against the float64 softmax over the
    EXPANDED incidence.  Tolerance: RTOL / ATOL, the PMA kernels' own."""
    from allset_amd import LeaveOneOutIncidence, pma_aggregate_exclude_self
    n_v, n_e, ei = _hypergraph(graph)
    eie, _ = _expanded(n_v, n_e, ei)
    ev, ep = eie[0].to(device), (eie[1] - n_v).to(device)
    loo = LeaveOneOutIncidence(ei.to(device), n_v=n_v, e_base=n_v)
    nnz, d = loo.nnz, 64
    A = torch.zeros(nnz, n_v, dtype=torch.bool, device=device)
    A[ep, ev] = True
    B = A.t()[:loo.n_dst].contiguous()
    g = torch.Generator().manual_seed(9 + heads)
    for direction, n_in, mask in (("v2e", n_v, A), ("e2v", nnz, B)):
        V = torch.randn(n_in, d, generator=g).to(device)
        alpha = (1.5 * torch.randn(n_in, heads, generator=g)).to(device)
        G = torch.randn(mask.shape[0], d, generator=g).to(device)
        Vg, ag = V.clone().requires_grad_(True), alpha.clone().requires_grad_(True)
        out = pma_aggregate_exclude_self(Vg, ag, loo, direction, heads, SLOPE)
        gV, ga = torch.autograd.grad(out, (Vg, ag), G)
        V64, a64 = V.double().requires_grad_(True), alpha.double().requires_grad_(True)
        ref = _dense_pma64(V64, a64, mask, heads)
        rV, ra = torch.autograd.grad(ref, (V64, a64), G.double())
        assert out.shape == ref.shape
        for what, got, want in (("forward", out.detach(), ref.detach()), ("grad V", gV, rV), ("grad alpha", ga, ra)):
            u = _units(got, want)
            print(f"{graph} H={heads} {direction} {what}: worst error {u:.4f} tolerance units")
            assert u <= 1.0, (direction, what, u)


# ---- (d) model parity --------------------------------------------------------------------------------------------------------------------
def _run_model(args, sd, data, device, name):
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


def _model_pair(device, mode, layers):
    from allset_amd import SetGNN
    from allset_amd import preprocessing as P
    n_v, n_e, ei = _hypergraph("small")
    F, hidden, C = 24, 64, 5
    args = cases.make_args(mode, F, hidden, C, All_num_layers=layers)
    spec = [(k, tuple(v.shape)) for k, v in SetGNN(args).state_dict().items()]
    sd = {k: torch.from_numpy(v) for k, v in cases.make_state_dict(spec, 23 + layers, kinkfree=True).items()}
    x = torch.from_numpy(np.random.default_rng(layers).standard_normal((n_v, F)).astype(np.float32))
    eie, norm = _expanded(n_v, n_e, ei)
    expanded = SimpleNamespace(x=x.clone().to(device).requires_grad_(True), edge_index=eie.to(device), norm=norm.to(device))
    plain = P.exclude_self(SimpleNamespace(x=x.clone().to(device).requires_grad_(True), edge_index=ei.clone().to(device),
                                           n_x=[n_v], num_hyperedges=[n_e]), attention=True)
    return args, sd, plain, expanded


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("mode", ["pma_h1", "pma_h4"])
def test_model_parity_with_the_expanded_model(device, mode, layers):
    """The same state_dict on unexpanded exclude-self data (attention=True) and on the expanded data: logits, the first layer's conv
    outputs, the input gradient and EVERY parameter gradient (fp32, rtol = atol = 1e-4 of each tensor's scale, as the Deep Sets test)."""
    args, sd, plain, expanded = _model_pair(device, mode, layers)
    want = _run_model(args, sd, expanded, device, f"loo_{mode}_L{layers}")
    got = _run_model(args, sd, plain, device, f"loo_{mode}_L{layers}")
    assert list(got["model"].state_dict()) == list(want["model"].state_dict())
    g = {"out_" + k: want[k].numpy() for k in ("logits", "v2e0", "e2v0", "grad_x")}
    g.update({"n_rows_" + k: np.int64(want[k].shape[0]) for k in ("logits", "v2e0", "e2v0")})
    g.update({"grad_" + k: v.numpy() for k, v in want["grads"].items()})
    assert got["v2e0"].shape[0] == plain.edge_index.shape[1]          # hyperedge-side activations: one row per incidence
    assert any(float(v.abs().max()) > 0 for v in want["grads"].values())
    util.assert_matches_golden(got, g, False, rtol=1e-4, atol=1e-4)


# ---- (e) hipGraph ---------------------------------------------------------------------------------------------------------------------------
def test_graphed_train_step_equals_eager(device):
    """The new path captures (nothing in it synchronises): three replayed steps equal three eager steps."""
    from allset_amd import SetGNN, dense
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    args, sd, plain, _ = _model_pair(device, "pma_h4", 2)
    plain.x = plain.x.detach()
    model = SetGNN(args)
    model.load_state_dict(sd)
    model.to(device)
    n_out = int(plain.edge_index[0].max()) + 1
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


# ---- (f) refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals(device):
    from allset_amd import LeaveOneOutIncidence, SetGNN, _lib, ops, pma_aggregate_exclude_self
    from allset_amd import preprocessing as P
    n_v, n_e, ei = _hypergraph("small")
    loo = LeaveOneOutIncidence(ei.to(device), n_v=n_v, e_base=n_v)
    V, alpha = torch.randn(n_v, 64, device=device), torch.randn(n_v, 4, device=device)
    for d, H in ((66, 1), (64, 3), (516, 1), (24, 4)):                # C % 4 != 0, heads not built, too wide, C = 6
        with pytest.raises(_lib.AllSetHipError, match="not built"):
            ops.loo_softmax_fwd(loo.e_rowptr, loo.e_col, torch.randn(n_v, H, device=device), torch.randn(n_v, d, device=device), H)
        with pytest.raises(_lib.AllSetHipError, match="not built"):
            pma_aggregate_exclude_self(torch.randn(n_v, d, device=device), torch.randn(n_v, H, device=device), loo, "v2e", H)
    with pytest.raises(_lib.AllSetHipError):
        ops.loo_softmax_fwd(loo.e_rowptr, loo.e_col, alpha.cpu(), V.cpu(), 4)          # no CPU fallback
    with pytest.raises(_lib.AllSetHipError):
        pma_aggregate_exclude_self(V.cpu(), alpha.cpu(), loo, "v2e", 4)
    with pytest.raises(NotImplementedError, match="expand"):
        pma_aggregate_exclude_self(V.bfloat16(), alpha, loo, "v2e", 4)
    with pytest.raises(NotImplementedError, match="expand"):
        ops.loo_softmax_fwd(loo.e_rowptr, loo.e_col, alpha, V.bfloat16(), 4)
    with pytest.raises(ValueError):
        pma_aggregate_exclude_self(V, alpha, loo, "sideways", 4)
    with pytest.raises(ValueError):
        pma_aggregate_exclude_self(V, alpha, loo, "e2v", 4)                            # E->V takes one row per incidence
    mk = lambda **kw: P.exclude_self(SimpleNamespace(x=torch.randn(n_v, 24, device=device), edge_index=ei.clone().to(device), n_x=[n_v],
                                                     num_hyperedges=[n_e]), **kw)
    pma = SetGNN(cases.make_args("pma_h1", 24, 64, 5)).to(device).eval()
    with pytest.raises(NotImplementedError, match="attention=True"):
        pma(mk())                                                                      # the default still refuses, and names the keyword
    assert pma(mk(attention=True)).shape[1] == 5
    margs = cases.make_args("pma_h1", 24, 64, 5, LearnMask=True)
    masked = SetGNN(margs, norm=torch.ones(ei.shape[1])).to(device).eval()
    with pytest.raises(NotImplementedError, match="LearnMask"):
        masked(mk(attention=True))
