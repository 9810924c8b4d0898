"""GPU: the sparse-hop kernels over adversarial row structures and every dispatch width (tests/hop_structures.py: graphs smaller than
a workgroup's four waves, rectangular ones, everything in one row / from one source, heavy duplication, runs of empty rows at both
ends, row lengths on the 64-incidence chunk boundary and on the families' long-row thresholds; widths on both sides of every lane-group
boundary), each against the float64 restatement that already lives in tests/*_oracle.py: the output and every gradient the function
declares differentiable, under ``(y * G).sum().backward()``.

The case lists are fixed and imported from tests/hop_structures.py; tests/test_hop_structures_host.py asserts on the CPU, from the
restatements alone, that every one of them has a finite reference, a leaky-relu logit margin of 1/16 and a relu pre-activation margin
of 0.25, so a mismatch here is the kernel's.  Tolerance: the families' own rule (rtol 1e-4, atol 1e-4 * max(1, max |want|)), which
their kernel-level tests hold on rows of 1500 to 4096 terms (the exclude-self functions: that family's own bound and the PMA kernels'
1e-4 units, as tests/test_gpu_exclude_self*.py).  One gradient of one case needs more; its slack comes from the float64 reference
alone (hop_structures.HAN_GEL_SLACK).  Dropout masks are rebuilt with ``dense.dropout_scale`` from the recorded seeds."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hop_structures as hs  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_INCS = {}


def _inc(name, T=hs.CSR_LONG_T):
    """The structure's :class:`Incidence` (sources -> targets), built once."""
    if (name, T) not in _INCS:
        from allset_amd import Incidence
        n_src, n_dst, ei = hs.structures(T)[name]
        _INCS[(name, T)] = Incidence.from_edge_index(torch.from_numpy(ei).to(DEV), n_src=n_src, n_dst=n_dst)
    return _INCS[(name, T)]


def _seeds(monkeypatch):
    from allset_amd import dense
    seeds = []
    real = dense._draw_seed
    monkeypatch.setattr(dense, "_draw_seed", lambda: seeds.append(real()) or seeds[-1])
    return seeds


def _mask(shape, p, seed):
    from allset_amd import dense
    return dense.dropout_scale(tuple(shape), p, seed, DEV).cpu().double()


def _dev(t, grad=False):
    return None if t is None else t.float().to(DEV).requires_grad_(grad)


def _grad(t):
    return t.grad if t.grad is not None else torch.zeros_like(t)


# ---- family 1: scaled_propagate, weighted_propagate ----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hs.HCONV_CASES, ids=lambda c: c.id)
def test_hconv_propagate_vs_float64(monkeypatch, c):
    from allset_amd.functional import scaled_propagate, weighted_propagate
    inp = hs.hconv_inputs(c)
    inc = _inc(c.struct)
    seeds = _seeds(monkeypatch)
    xd, bd = _dev(inp["x"], True), _dev(inp["b"], True)
    if c.weighted:
        w = _dev(inp["w"])
        w_dst = w.index_select(0, inc.perm_dst_long()) if w is not None else None
        w_src = w.index_select(0, inc.perm_src_long()) if w is not None else None
        y = weighted_propagate(xd, inc, w_dst, w_src, bias=bd, act=c.act, p=c.p, variant=c.variant)
    else:
        y = scaled_propagate(xd, inc, c.direction, r=_dev(inp["r"]), s=_dev(inp["s"]), bias=bd, act=c.act, p=c.p, variant=c.variant)
    (y * _dev(inp["G"])).sum().backward()
    assert len(seeds) == (c.p > 0)
    mask = _mask((inp["n_t"], c.d), c.p, seeds[0]) if c.p > 0 else None
    yo, grads, _ = hs.hconv_reference(c, inp, mask)
    hs.close(y, yo, "y")
    hs.close(_grad(xd), grads["gx"], "gx")
    hs.close(_grad(bd), grads["gb"], "gbias")


@pytest.mark.parametrize("name,d", hs.HCONV_VARIANT_ERRORS)
def test_forced_short_row_variant_is_refused_outside_its_domain(name, d):
    from allset_amd._lib import AllSetHipError
    from allset_amd.functional import scaled_propagate, weighted_propagate
    inc = _inc(name)
    x = torch.ones(inc.n_src, d, device=DEV)
    for call in (lambda: scaled_propagate(x, inc, "v2e", variant=2), lambda: weighted_propagate(x, inc, None, None, variant=2)):
        with pytest.raises(AllSetHipError, match=hs.HCONV_VARIANT_MESSAGE):
            call()
    with pytest.raises(AllSetHipError, match="variant must be None, 1 or 2"):
        scaled_propagate(x, inc, "v2e", variant=3)
    torch.testing.assert_close(scaled_propagate(x, inc, "v2e", variant=1), scaled_propagate(x, inc, "v2e"))     # the device is usable


def test_variant_none_is_the_csrs_own_choice_bit_for_bit():
    """At dataset scale (<= 16384 rows) the CSR picks one wavefront per row: ``variant=None`` equals a forced 1, bit for bit, in the
    output and in the gradient; the short-row kernel sums a row in another order and need not."""
    from allset_amd.functional import scaled_propagate
    inc = _inc("flat50")
    assert inc.by_dst.variant("segreduce", inc.n_dst) == 1 and inc.by_src.variant("segreduce", inc.n_src) == 1
    g = torch.Generator().manual_seed(3)
    x = torch.randn(inc.n_src, 64, generator=g)
    r, s, b = torch.rand(inc.n_src, generator=g).to(DEV), torch.rand(inc.n_dst, generator=g).to(DEV), torch.randn(64, generator=g).to(DEV)
    outs = []
    for variant in (None, 1):
        xd = x.to(DEV).requires_grad_(True)
        y = scaled_propagate(xd, inc, "v2e", r=r, s=s, bias=b, act="elu", variant=variant)
        y.square().sum().backward()
        outs.append((y.detach(), xd.grad))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- family 2: gat_propagate ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hs.GAT_CASES, ids=lambda c: c.id)
def test_gat_propagate_vs_float64(monkeypatch, c):
    from allset_amd.functional import gat_propagate
    inp = hs.gat_inputs(c)
    inc = _inc(c.struct)
    seeds = _seeds(monkeypatch)
    dv = [_dev(inp[k], True) for k in ("x", "al", "ar", "b")]
    y = gat_propagate(dv[0], dv[1], dv[2], inc, c.H, 0.2, c.concat, bias=dv[3], act=c.act, p=c.p)
    (y * _dev(inp["G"])).sum().backward()
    mask = _mask(y.shape, c.p, seeds[0]) if c.p > 0 else None
    yo, grads, _, _ = hs.gat_reference(c, inp, mask)
    hs.close(y, yo, "y")
    if c.p == 0:                                                           # the forward nobody differentiates is another instantiation
        x0, al0, ar0, b0 = (t.detach() for t in dv)
        hs.close(gat_propagate(x0, al0, ar0, inc, c.H, 0.2, c.concat, bias=b0, act=c.act), yo, "y (no grad)")
    for t, k in zip(dv, ("gx", "gal", "gar", "gb")):
        hs.close(_grad(t), grads[k], k)
    empty = torch.bincount(inp["ei"][1], minlength=inp["n_dst"]) == 0
    if bool(empty.any()):                                                  # an empty target row leaves with act(bias) alone
        want = inp["b"].clamp(min=0) if c.act == "relu" else inp["b"]
        want = want.expand(int(empty.sum()), -1) * (mask[empty] if mask is not None else 1.0)
        torch.testing.assert_close(y.detach().cpu().double()[empty], want.float().double(), rtol=1e-6, atol=0)


# ---- family 3: hattn_propagate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hs.HATTN_CASES, ids=lambda c: c.id)
def test_hattn_propagate_vs_float64(monkeypatch, c):
    from allset_amd import hattn_propagate
    inp = hs.hattn_inputs(c)
    inc = _inc(c.struct)
    nnz = inp["ei"].shape[1]
    seeds = _seeds(monkeypatch)
    dv = [_dev(inp[k], True) for k in ("z", "av", "ae", "b")]
    y = hattn_propagate(dv[0], dv[1], dv[2], inc, c.H, _dev(inp["D"]), _dev(inp["B"]), 0.2, c.concat, bias=dv[3], act=c.act,
                        p_attn=c.p_attn, p=c.p)
    (y * _dev(inp["G"])).sum().backward()
    assert len(seeds) == (c.p_attn > 0) + (c.p > 0)
    cm = _mask((nnz, c.H), c.p_attn, seeds[0]) if (c.p_attn > 0 and nnz) else None
    om = _mask(y.shape, c.p, seeds[-1]) if c.p > 0 else None
    yo, grads, _, _ = hs.hattn_reference(c, inp, cm, om)
    hs.close(y, yo, "y")
    for t, k in zip(dv, ("gz", "gav", "gae", "gb")):
        hs.close(_grad(t), grads[k], k)
    iso = torch.bincount(inp["ei"][0], minlength=inp["n_v"]) == 0
    if bool(iso.any()):                                                    # an isolated vertex: nothing reaches it, nothing leaves it
        assert float(_grad(dv[0])[iso.to(DEV)].abs().max()) == 0.0


# ---- family 4: unignn_hop, unigat_edge, unigcn_hop -----------------------------------------------------------------------------------
@pytest.mark.parametrize("c", hs.UNIGNN_CASES, ids=lambda c: c.id)
def test_unignn_hop_vs_float64(monkeypatch, c):
    from allset_amd import ops
    from allset_amd.functional import unignn_hop
    inp = hs.unignn_inputs(c)
    inc = _inc(c.struct)
    seeds = _seeds(monkeypatch)
    dxe, dxs = _dev(inp["xe"], True), _dev(inp["xs"], True)
    dc = torch.tensor([hs.UNIGNN_C], device=DEV, requires_grad=True)
    assert ops.unignn_hop_supported(dxe, dxs) == hs.uni_fused(c.d)        # (False: the documented unfused composition runs below)
    kw = dict(s=_dev(inp["s"]), use_norm=c.use_norm, act=c.act, p=c.p, variant=c.variant)
    if c.self_term != "none":
        kw.update(xs=dxs, c=dc if c.self_term == "tensor" else 1.0)
    y = unignn_hop(dxe, inc, **kw)
    (y * _dev(inp["G"])).sum().backward()
    mask = _mask((inp["n_v"], c.d), c.p, seeds[0]) if c.p > 0 else None
    yo, grads, t, _ = hs.unignn_reference(c, inp, mask)
    hs.close(y, yo, "y")
    hs.close(_grad(dxe), grads["gxe"], "gxe")
    if c.self_term != "none":
        hs.close(_grad(dxs), grads["gxs"], "gxs")
    if c.self_term == "tensor":
        hs.close(_grad(dc), grads["gc"], "gc")
    iso = torch.bincount(inp["ei"][0], minlength=inp["n_v"]) == 0
    if c.use_norm and c.self_term == "none" and bool(iso.any()):          # the norm of an exactly-zero row: t = 0, the row stays 0
        assert float(y.detach()[iso.to(DEV)].abs().max()) == 0.0


@pytest.mark.parametrize("c", hs.UNIGAT_CASES, ids=lambda c: c.id)
def test_unigat_edge_vs_float64(c):
    from allset_amd import ops
    from allset_amd.functional import unigat_edge
    inp = hs.unigat_inputs(c)
    inc = _inc(c.struct)
    dx, datt = _dev(inp["x"], True), _dev(inp["att"], True)
    assert ops.unignn_v2e_att_supported(dx, c.H) == hs.uni_fused(c.H * c.C, c.C)
    xe, ae = unigat_edge(dx, inc, _dev(inp["s"]), datt, c.H, variant=c.variant)
    ((xe * _dev(inp["G"])).sum() + (ae * _dev(inp["Ga"])).sum()).backward()
    xo, ao, grads = hs.unigat_reference(c, inp)
    hs.close(xe, xo, "xe")
    hs.close(ae, ao, "ae")
    hs.close(_grad(dx), grads["gx"], "gx")
    hs.close(_grad(datt), grads["gatt"], "gatt")


@pytest.mark.parametrize("c", hs.UNIGCN_CASES, ids=lambda c: c.id)
def test_unigcn_hop_vs_float64(c):
    from allset_amd import ops
    from allset_amd.functional import unigcn_hop
    inp = hs.unigcn_inputs(c)
    inc = _inc(c.struct)
    dxe, dx0 = _dev(inp["xe"], True), _dev(inp["x0"], True)
    assert ops.unigcn_hop_supported(dxe, dx0) == hs.uni_fused(c.d)
    xi = unigcn_hop(dxe, dx0, inc, _dev(inp["degV"]), hs.UNIGCN_ALPHA, c.use_norm, variant=c.variant)
    (xi * _dev(inp["G"])).sum().backward()
    xo, grads = hs.unigcn_reference(c, inp)
    hs.close(xi, xo, "xi")
    hs.close(_grad(dxe), grads["gxe"], "gxe")
    hs.close(_grad(dx0), grads["gx0"], "gx0")


@pytest.mark.parametrize("name,d", hs.UNI_VARIANT_ERRORS)
def test_uni_forced_short_row_variant_is_refused_above_256_columns(name, d):
    from allset_amd._lib import AllSetHipError
    from allset_amd.functional import unigat_edge, unigcn_hop, unignn_hop
    inc = _inc(name)
    xe, x = torch.ones(inc.n_dst, d, device=DEV), torch.ones(inc.n_src, d, device=DEV)
    for call in (lambda: unignn_hop(xe, inc, variant=2), lambda: unigcn_hop(xe, x, inc, torch.ones(inc.n_src, device=DEV), 0.1, False, variant=2),
                 lambda: unigat_edge(x, inc, None, torch.ones(d, device=DEV), 1, variant=2)):
        with pytest.raises(AllSetHipError, match=hs.UNI_SHORT_ROW_MESSAGE):
            call()
    torch.testing.assert_close(unignn_hop(xe, inc, variant=1), unignn_hop(xe, inc))                     # the device is usable


# ---- family 5: han_gat_propagate, han_block_propagate ----------------------------------------------------------------------------------
_HAN_GRAPHS = {}


def _han_graph(name, block):
    if (name, block) not in _HAN_GRAPHS:
        from allset_amd.han import MetapathGraph
        from allset_amd.han_sampling import Block
        n_src, n_dst, src, dst = hs.han_edges(name, block)
        _HAN_GRAPHS[(name, block)] = Block.from_edges(src.to(DEV), dst.to(DEV), n_src, n_dst) if block else \
            MetapathGraph(src.to(DEV), dst.to(DEV), n_dst)
    return _HAN_GRAPHS[(name, block)]


@pytest.mark.parametrize("c", hs.HAN_CASES, ids=lambda c: c.id)
def test_han_propagate_vs_float64(monkeypatch, c):
    from allset_amd.functional import han_block_propagate, han_edge_keep, han_gat_propagate
    inp = hs.han_inputs(c)
    graph = _han_graph(c.struct, c.block)
    seeds = _seeds(monkeypatch)
    dv = [_dev(inp[k], True) for k in ("x", "el", "er", "b")]
    fn = han_block_propagate if c.block else han_gat_propagate
    y = fn(dv[0], dv[1], dv[2], graph, c.H, 0.2, bias=dv[3], attn_drop=c.p)
    (y * _dev(inp["G"])).sum().backward()
    keep = han_edge_keep(graph, c.H, c.p, seeds[0]).cpu().double() if c.p > 0 else None
    yo, grads, _ = hs.han_reference(c, inp, keep)
    hs.close(y, yo, "y")
    if c.p == 0:                                                           # the forward nobody differentiates is another instantiation
        x0, el0, er0, b0 = (t.detach() for t in dv)
        hs.close(fn(x0, el0, er0, graph, c.H, 0.2, bias=b0), yo, "y (no grad)")
    for t, k in zip(dv, ("gx", "gel", "ger", "gb")):
        slack = hs.han_gel_slack(c, inp, keep) if (k == "gel" and c.id in hs.HAN_GEL_SLACK) else None
        hs.close(_grad(t), grads[k], k, slack)


@pytest.mark.parametrize("name", hs.HAN_BLOCK_ERRORS)
def test_a_block_with_more_targets_than_sources_is_refused(name):
    from allset_amd.han_sampling import Block
    n_src, n_dst, ei = hs.structures()[name]
    assert n_dst > n_src
    with pytest.raises(ValueError, match=hs.HAN_BLOCK_ERROR):
        Block.from_edges(torch.from_numpy(ei[0].copy()).to(DEV), torch.from_numpy(ei[1].copy()).to(DEV), n_src, n_dst)


# ---- family 6: clique_propagate --------------------------------------------------------------------------------------------------------
_CE_GRAPHS = {}


def _ce_graph(name):
    if name not in _CE_GRAPHS:
        from allset_amd.baselines import ImplicitCEGraph
        n_v, _, ei = hs.structures(hs.LOO_LONG_T)[name]
        _CE_GRAPHS[name] = ImplicitCEGraph(torch.from_numpy(ei).to(DEV), n_v)
    return _CE_GRAPHS[name]


@pytest.mark.parametrize("c", hs.CLIQUE_CASES, ids=lambda c: c.id)
def test_clique_propagate_vs_float64(monkeypatch, c):
    from allset_amd import ops
    from allset_amd.functional import clique_propagate
    assert ops.loo_long_threshold() == hs.LOO_LONG_T                      # the threshold ``lengths`` was built around
    inp = hs.clique_inputs(c)
    graph = _ce_graph(c.struct)
    seeds = _seeds(monkeypatch)
    xd, bd = _dev(inp["x"], True), _dev(inp["b"], True)
    y = clique_propagate(xd, graph, bias=bd, act=c.act, p=c.p)
    (y * _dev(inp["G"])).sum().backward()
    mask = _mask((inp["n_v"], c.d), c.p, seeds[0]) if c.p > 0 else None
    yo, grads, _ = hs.clique_reference(c, inp, mask)
    hs.close(y, yo, "y")
    hs.close(_grad(xd), grads["gx"], "gx")
    hs.close(_grad(bd), grads["gb"], "gbias")


@pytest.mark.parametrize("name", hs.CLIQUE_NO_PAIR)
def test_a_list_without_a_pair_has_no_clique_expansion(name):
    from allset_amd.baselines import ImplicitCEGraph
    n_v, _, ei = hs.structures()[name]
    with pytest.raises(ValueError, match=hs.CLIQUE_EMPTY_MESSAGE):
        ImplicitCEGraph(torch.from_numpy(ei).to(DEV), n_v)


# ---- family 7: deepsets_aggregate_exclude_self, pma_aggregate_exclude_self ---------------------------------------------------------------
_LOOS = {}


def _loo(name):
    if name not in _LOOS:
        from allset_amd import LeaveOneOutIncidence
        n_v, _, ei = hs.loo_list(name)
        _LOOS[name] = LeaveOneOutIncidence(ei.to(DEV), n_v=n_v, e_base=n_v)
    return _LOOS[name]


@pytest.mark.parametrize("c", [c for c in hs.LOO_CASES if c.kind == "ds"], ids=lambda c: c.id)
def test_deepsets_exclude_self_vs_the_expansion_in_float64(c):
    """Both directions, forward and input gradient, against the float64 product with the dense expanded incidence, under the
    exclude-self family's own bound (tests/test_gpu_exclude_self.py)."""
    from allset_amd import deepsets_aggregate_exclude_self, ops
    assert ops.loo_long_threshold() == hs.LOO_LONG_T
    inp = hs.loo_inputs(c)
    loo = _loo(c.struct)
    A, B, terms_e, terms_v = hs.loo_matrices(c.struct, c.aggr, c.normtype)
    assert (loo.nnz, loo.n_dst) == (A.shape[0], B.shape[0])
    xv = _dev(inp["x"], True)
    out = deepsets_aggregate_exclude_self(xv, loo, "v2e", c.aggr, c.normtype)
    (gx,) = torch.autograd.grad(out, xv, _dev(inp["G_e"]))
    hs.loo_bound_check(out, A, inp["x"], terms_e, "v2e forward")
    hs.loo_bound_check(gx, A.t(), inp["G_e"], terms_v, "v2e input gradient")
    yv = _dev(inp["y"], True)
    out = deepsets_aggregate_exclude_self(yv, loo, "e2v", c.aggr, c.normtype)
    (gy,) = torch.autograd.grad(out, yv, _dev(inp["G_v"]))
    hs.loo_bound_check(out, B, inp["y"], terms_v, "e2v forward")
    hs.loo_bound_check(gy, B.t(), inp["G_v"], terms_e, "e2v input gradient")


@pytest.mark.parametrize("c", [c for c in hs.LOO_CASES if c.kind == "pma"], ids=lambda c: c.id)
def test_pma_exclude_self_vs_the_dense_softmax_in_float64(c):
    """Both directions, forward and the gradients to V and alpha, against the float64 softmax over the EXPANDED incidence, at the PMA
    kernels' own tolerance (tests/test_gpu_exclude_self_pma.py)."""
    from allset_amd import pma_aggregate_exclude_self
    inp = hs.loo_inputs(c)
    loo = _loo(c.struct)
    ref = hs.loo_pma_reference(c, inp)
    for direction, V, al, G in (("v2e", inp["x"], inp["ax"], inp["G_e"]), ("e2v", inp["y"], inp["ay"], inp["G_v"])):
        Vg, ag = _dev(V, True), _dev(al, True)
        out = pma_aggregate_exclude_self(Vg, ag, loo, direction, c.H, 0.2)
        gV, ga = torch.autograd.grad(out, (Vg, ag), _dev(G), allow_unused=True)
        for what, got, want in (("forward", out, ref[direction][0]), ("grad V", gV, ref[direction][1]), ("grad alpha", ga, ref[direction][2])):
            got = torch.zeros_like(want) if got is None else got
            u = hs.units(got, want)
            print(f"{direction} {what}: worst error {u:.4f} tolerance units")
            assert u <= 1.0, (direction, what, u)


@pytest.mark.parametrize("name", hs.LOO_DUPLICATES)
def test_a_repeated_pair_has_no_exclude_self_expansion(name):
    from allset_amd import LeaveOneOutIncidence
    n_v, _, ei = hs.loo_list(name)
    with pytest.raises(ValueError, match=hs.LOO_DUPLICATE_MESSAGE):
        LeaveOneOutIncidence(ei.to(DEV), n_v=n_v, e_base=n_v)


@pytest.mark.parametrize("kind,H,C", hs.LOO_UNBUILT)
def test_an_unbuilt_exclude_self_width_raises_and_has_no_fallback(kind, H, C):
    from allset_amd import deepsets_aggregate_exclude_self, pma_aggregate_exclude_self
    from allset_amd._lib import AllSetHipError
    loo = _loo("flat50")
    x = torch.ones(loo.n_v, H * C, device=DEV)
    with pytest.raises(AllSetHipError, match="is not built"):
        if kind == "ds":
            deepsets_aggregate_exclude_self(x, loo, "v2e")
        else:
            pma_aggregate_exclude_self(x, torch.ones(loo.n_v, H, device=DEV), loo, "v2e", H)
