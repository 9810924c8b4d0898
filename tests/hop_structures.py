"""Row structures, width classes, kink-free inputs and the fixed case lists of the sparse-hop sweep.  Imports on the CPU; shared by
tests/test_hop_structures_host.py (which vouches for every case from the float64 restatements alone) and
tests/test_gpu_hop_structures.py (which runs the same lists through the HIP kernels), so the two cannot drift.

Structures are ``(n_src, n_dst, edge_index)`` with ``edge_index`` int64 ``[2, nnz]`` (row 0 sources, row 1 targets), built from
``numpy.random.default_rng`` with fixed seeds, at the smallest size at which the edge exists (no side above 700 rows, nnz <= ~6000).

Inputs keep clear of the kinks by construction, never by a seed search:
  * attention logit terms are multiples of 1/8, the target-side term carries an additional 1/16: every ``al[s] + ar[t]`` is an odd
    multiple of 1/16, exact in fp32, at least 1/16 from leaky_relu's kink;
  * under a relu epilogue column ``c`` of every input row and of the bias carries one sign (alternating with ``c mod C``) and a
    magnitude of at least 0.25; scales, softmax weights and dropout factors are non-negative, so every pre-activation keeps the sign
    and at least the bias' magnitude.  Both relu branches are exercised (even columns positive, odd ones negative);
  * elu or no activation: plain ``randn``.
All values are fp32-representable float64."""
from __future__ import annotations

import itertools
import os
import sys
from collections import OrderedDict, namedtuple

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import baselines_oracle  # noqa: E402
import cegat_oracle  # noqa: E402
import hcha_attn_oracle  # noqa: E402

D64 = torch.float64
LOGIT_MARGIN = 1.0 / 16
RELU_MARGIN = 0.25

# The row-length thresholds of the code (never guessed):
#   * exclude-self / scan families: ``ops.loo_long_threshold()`` (csrc/loo.hip kLooLong; csrc/loo_softmax.hip and csrc/scan.hip share
#     the same long-segment list) -- read from the library where it is loaded, and pinned against this literal by the GPU file;
#   * the CSR hops (hconv, gat, hattn, unignn, unigcn, han) have ONE kernel for every row length -- a row is walked in 64-incidence
#     chunks -- and the only row-length rule on their path is ``ops.long_rows_first_order``'s ``max_deg > 256`` (the dispatch order of
#     a skewed CSR).  The host file pins that literal by calling the function on both sides of it.
LOO_LONG_T = 64
CSR_LONG_T = 256
_LENGTHS = (0, 0, 1, 9, 0, 0, 0, 17, 2, 63, 64, 65, 0, 127, 128, 129, 1, 0, "T-1", "T", "T+1", 0, 0)


def lengths_rows(T):
    return [({"T-1": T - 1, "T": T, "T+1": T + 1}[v] if isinstance(v, str) else v) for v in _LENGTHS]


def _rows_to_edges(rng, n_src, row_lengths):
    """Target row t gets ``row_lengths[t]`` distinct sources."""
    src, dst = [], []
    for t, L in enumerate(row_lengths):
        if L:
            src.append(rng.choice(n_src, size=L, replace=False))
            dst.append(np.full(L, t))
    if not src:
        return np.zeros((2, 0), dtype=np.int64)
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    return ei[:, rng.permutation(ei.shape[1])]                      # edge-list order is not CSR order


def structures(T=CSR_LONG_T):
    """name -> (n_src, n_dst, edge_index int64 [2, nnz] numpy).  ``T``: the family's long-row threshold (``lengths`` only)."""
    out = OrderedDict()
    out["empty"] = (5, 3, np.zeros((2, 0), dtype=np.int64))
    out["single"] = (1, 1, np.zeros((2, 1), dtype=np.int64))
    out["tiny"] = (3, 2, np.array([[0, 1, 2, 1], [0, 0, 0, 1]], dtype=np.int64))
    out["rows5"] = (6, 5, _rows_to_edges(np.random.default_rng(105), 6, [4] * 5))           # 4 waves' rows plus one
    rng = np.random.default_rng(106)
    one_row = np.stack([rng.integers(0, 300, size=1500), np.full(1500, 17)]).astype(np.int64)
    out["one_row"] = (300, 37, one_row)
    out["one_col"] = (37, 300, one_row[::-1].copy())
    rng = np.random.default_rng(107)
    key = rng.choice(40 * 30, size=50, replace=False)
    pairs = np.stack([key // 30, key % 30]).astype(np.int64)
    out["dups"] = (40, 30, np.repeat(pairs, 8, axis=1)[:, rng.permutation(400)])
    rng = np.random.default_rng(108)
    ee = _rows_to_edges(rng, 75, [0] * 3 + [int(v) for v in rng.integers(1, 13, size=57)] + [0] * 40)
    ee[0] += 5                                                      # the transposed side too: sources 0..4 and 80..89 are isolated
    out["edge_empties"] = (90, 100, ee)
    rng = np.random.default_rng(109)
    out["wide"] = (700, 9, _rows_to_edges(rng, 700, [int(v) for v in rng.integers(200, 400, size=9)]))
    rng = np.random.default_rng(110)
    out["tall"] = (9, 700, _rows_to_edges(rng, 9, [int(v) for v in rng.integers(0, 4, size=700)]))
    out["lengths"] = (max(300, T + 44), len(_LENGTHS), _rows_to_edges(np.random.default_rng(111), max(300, T + 44), lengths_rows(T)))
    rng = np.random.default_rng(112)
    out["flat50"] = (60, 50, _rows_to_edges(rng, 60, list(_LENGTHS[:8]) + [int(v) for v in rng.integers(0, 8, size=42)]))
    return out


VEC_WIDTHS = (4, 12, 32, 36, 64, 68, 128, 132, 256, 260, 512)
SCALAR_WIDTHS = (1, 3, 7, 9, 18, 33, 70, 257)


def width_classes(vec_ok, built=lambda d: True):
    """The widths on both sides of every ``pick_lpr`` boundary (csrc/common.h): rows that take the 16-byte path (``vec_ok``) or the
    scalar one, cut to what the family builds."""
    return [d for d in (VEC_WIDTHS if vec_ok else SCALAR_WIDTHS) if built(d)]


def pick_lpr(d, vec):
    """csrc/common.h pick_lpr, restated for the coverage assertions of the host file."""
    need, lpr = (d + vec - 1) // vec, 8
    while lpr < need and lpr < 64:
        lpr *= 2
    return lpr


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _f32(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32)).double()


def randn(rng, *shape):
    return _f32(rng.standard_normal(shape))


def positive(rng, n):
    """Scales in [0.5, 1.5)."""
    return _f32(rng.random(n) + 0.5)


def signed_rows(rng, n, d, C=None):
    """[n, d]: column c has sign (-1)^(c mod C) and magnitude in [0.25, 1.75)."""
    C = d if C is None else C
    sign = np.where((np.arange(d) % C) % 2 == 0, 1.0, -1.0)
    return _f32((0.25 + 1.5 * rng.random((n, d))) * sign)


def logit_terms(rng, n, H, target):
    """Multiples of 1/8 in [-2, 2]; the target side carries an additional 1/16."""
    return _f32(rng.integers(-16, 17, size=(n, H)) / 8.0 + (LOGIT_MARGIN if target else 0.0))


def host_mask(shape, p, seed):
    """A stand-in for the library's hash mask where there is no device (host file): Bernoulli keep / (1 - p)."""
    if p <= 0:
        return None
    keep = np.random.default_rng(seed).random(shape) >= p
    return torch.from_numpy(keep / (1.0 - p)).double()


def close(got, want, what, slack=None):
    """The families' own rule (tests/test_gpu_cegat.py _close): rtol 1e-4, atol 1e-4 * max(1, max |want|).  ``slack``: an additional
    per-element absolute allowance, derived by the caller from the float64 reference alone (see HAN_GEL_SLACK)."""
    got = got.detach().cpu().double()
    want = want.detach()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} against {tuple(want.shape)}"
    scale = float(want.abs().max()) if want.numel() else 0.0
    err = float((got - want).abs().max()) if want.numel() else 0.0
    print(f"{what}: max |diff| {err:.3e}, max |want| {scale:.3e}")
    if slack is None:
        torch.testing.assert_close(got, want, rtol=1e-4, atol=1e-4 * max(1.0, scale),
                                   msg=lambda m: f"{what}: max |diff| {err:.3e} at max |want| {scale:.3e}: {m}")
    else:
        tol = 1e-4 * max(1.0, scale) + 1e-4 * want.abs() + slack
        worst = float(((got - want).abs() / tol).max()) if want.numel() else 0.0
        assert worst <= 1.0, f"{what}: max |diff| {err:.3e} at max |want| {scale:.3e}, max slack {float(slack.max()):.3e}: err / tol = {worst:.3f}"


def _cid(*parts):
    return "-".join(str(p) for p in parts)


def _sweep(widths_vec, widths_scalar):
    """(structure, width) pairs of one family: every structure at two widths, one per vector path (rotating through the width
    classes), and every width class at ``edge_empties`` and at ``lengths``."""
    names = list(structures())
    pairs = []
    for i, name in enumerate(names):
        pairs.append((name, widths_vec[i % len(widths_vec)]))
        pairs.append((name, widths_scalar[i % len(widths_scalar)]))
    for name in ("edge_empties", "lengths"):
        for d in list(widths_vec) + list(widths_scalar):
            if (name, d) not in pairs:
                pairs.append((name, d))
    return pairs


# ---- family 1: scaled_propagate / weighted_propagate (csrc/hconv.hip) ---------------------------------------------------------------
HconvCase = namedtuple("HconvCase", "id struct d weighted direction has_r has_s act p variant")


def hconv_flat_ok(d):
    """The short-row kernel's domain (csrc/hconv.hip: 16-byte rows, d <= 256)."""
    return d % 4 == 0 and d <= 256


def _hconv_cases():
    cases = []
    # scaled: direction x r x s x act x variant, walked in an order that changes every factor often
    combos = list(itertools.product(("v2e", "e2v"), (True, False), (True, False), (None, "relu", "elu"), (1, 2, None)))
    order = np.random.default_rng(201).permutation(len(combos))
    cyc = itertools.cycle([combos[i] for i in order])
    for name, d in _sweep(VEC_WIDTHS, SCALAR_WIDTHS):
        direction, has_r, has_s, act, variant = next(cyc)
        if variant == 2 and not hconv_flat_ok(d):
            variant = 1                                              # (the refusal of a forced 2 there: HCONV_VARIANT_ERRORS)
        cases.append(HconvCase(_cid("scaled", name, d, direction, "r" if has_r else "", "s" if has_s else "", act, f"v{variant}"),
                               name, d, False, direction, has_r, has_s, act, 0.0, variant))
    # every (LPR, scale form) of the short-row kernel over the two adversarial row structures, and plain AUTO over them
    for name in ("flat50", "lengths", "edge_empties"):
        for d in (12, 36, 68, 132):
            for has_r, has_s in ((True, False), (False, True)):
                cases.append(HconvCase(_cid("scaled", name, d, "v2e", "r" if has_r else "s", "relu", "v2"), name, d, False, "v2e", has_r,
                                       has_s, "relu", 0.0, 2))
    # dropout: odd and multiple-of-4 widths under the 8-bit (p = 0.5) and the 16-bit (p = 0.3) mask, both kernels
    for p in (0.5, 0.3):
        for name, d, variant in (("lengths", 7, 1), ("flat50", 33, 1), ("flat50", 36, 2), ("lengths", 260, 1), ("edge_empties", 12, 2)):
            for act in ("relu", "elu"):
                cases.append(HconvCase(_cid("scaled", name, d, act, f"p{p}", f"v{variant}"), name, d, False, "v2e", True, True, act, p, variant))
    # weighted: with and without weights, variant 1 and forced 2 (None: the CSR's own choice)
    wc = itertools.cycle(itertools.product((True, False), (None, "relu", "elu"), (1, 2, None)))
    for name, d in _sweep(VEC_WIDTHS, SCALAR_WIDTHS):
        has_w, act, variant = next(wc)
        if variant == 2 and not hconv_flat_ok(d):
            variant = 1
        cases.append(HconvCase(_cid("weighted", name, d, "w" if has_w else "", act, f"v{variant}"), name, d, True, "v2e", has_w, False,
                               act, 0.0, variant))
    for name in ("flat50", "lengths"):
        for d in (12, 36, 68, 132):
            cases.append(HconvCase(_cid("weighted", name, d, "w", "relu", "v2"), name, d, True, "v2e", True, False, "relu", 0.0, 2))
        for d in (12, 36, 68, 132):
            cases.append(HconvCase(_cid("weighted", name, d, "w", "elu", "v1", "rows"), name, d, True, "v2e", True, False, "elu", 0.0, 1))
    for p, d, variant in ((0.5, 9, 1), (0.5, 64, 2), (0.3, 3, 1), (0.3, 128, 2)):
        cases.append(HconvCase(_cid("weighted", "flat50", d, "w", "relu", f"p{p}", f"v{variant}"), "flat50", d, True, "v2e", True, False,
                               "relu", p, variant))
    assert len({c.id for c in cases}) == len(cases)
    return cases


HCONV_CASES = _hconv_cases()
# a forced short-row variant outside its domain is refused by the C entry (csrc/hconv.hip), not quietly served by the other kernel
HCONV_VARIANT_ERRORS = [("flat50", 3), ("flat50", 260), ("empty", 7)]
HCONV_VARIANT_MESSAGE = "the short-row variant needs 16-byte aligned rows and d <= 256"


def hconv_inputs(c):
    """float64 inputs of one case: ``x`` [n gathered, d], ``r`` (per gathered row) / ``s`` (per output row) or, weighted, ``w`` per
    incidence in edge-list order; bias (always: it carries the relu margin), cotangent ``G``."""
    n_src, n_dst, ei = structures()[c.struct]
    ei = torch.from_numpy(ei)
    rng = np.random.default_rng(abs(hash_id(c.id)))
    to_dst = c.direction == "v2e"
    n_s, n_t = (n_src, n_dst) if to_dst else (n_dst, n_src)
    relu = c.act == "relu"
    x = signed_rows(rng, n_s, c.d) if relu else randn(rng, n_s, c.d)
    b = signed_rows(rng, 1, c.d)[0] if relu else randn(rng, c.d)
    r = s = w = None
    if c.weighted:
        w = positive(rng, ei.shape[1]) if c.has_r else None
    else:
        r = positive(rng, n_s) if c.has_r else None
        s = positive(rng, n_t) if c.has_s else None
    return dict(n_src=n_src, n_dst=n_dst, n_s=n_s, n_t=n_t, ei=ei, x=x, r=r, s=s, w=w, b=b, G=randn(rng, n_t, c.d))


def hash_id(text):
    """A seed from a case id that does not depend on PYTHONHASHSEED."""
    h = 2166136261
    for ch in text.encode():
        h = ((h ^ ch) * 16777619) & 0x7FFFFFFF
    return h


def hconv_reference(c, inp, mask):
    """``(y, {'gx', 'gb'}, relu margin)`` from ``baselines_oracle.propagate``.  The weighted form is the same restatement over one
    gathered row per incidence (``x[src_j]``, scaled by ``w_j``)."""
    ei = inp["ei"]
    x = inp["x"].clone().requires_grad_(True)
    b = inp["b"].clone().requires_grad_(True)
    gi, oi = (ei[0], ei[1]) if c.direction == "v2e" else (ei[1], ei[0])

    def run(bias, act, m):
        if c.weighted:
            return baselines_oracle.propagate(x[gi], torch.arange(gi.numel()), oi, inp["n_t"], r=inp["w"], bias=bias, act=act, mask=m)
        return baselines_oracle.propagate(x, gi, oi, inp["n_t"], r=inp["r"], s=inp["s"], bias=bias, act=act, mask=m)
    y = run(b, c.act, mask)
    (y * inp["G"]).sum().backward()
    with torch.no_grad():
        pre = run(b, None, None)
    margin = float(pre.abs().min()) if c.act == "relu" else float("inf")
    gx = x.grad if x.grad is not None else torch.zeros_like(x)
    return y.detach(), dict(gx=gx, gb=b.grad), margin


# ---- family 2: gat_propagate (csrc/gat.hip) ----------------------------------------------------------------------------------------
GatCase = namedtuple("GatCase", "id struct H C concat act p")
# (H, C) of every width class: C % 4 == 0 takes the 16-byte path, anything else the scalar one
GAT_VEC_HC = OrderedDict([(4, (1, 4)), (12, (3, 4)), (32, (2, 16)), (36, (3, 12)), (64, (4, 16)), (68, (1, 68)), (128, (8, 16)),
                          (132, (3, 44)), (256, (4, 64)), (260, (5, 52)), (512, (8, 64))])
GAT_SCALAR_HC = OrderedDict([(1, (1, 1)), (3, (3, 1)), (7, (1, 7)), (9, (3, 3)), (18, (2, 9)), (33, (3, 11)), (70, (2, 35)),
                             (257, (1, 257))])


def _gat_cases():
    cases = []
    hc = dict(GAT_VEC_HC)
    hc.update(GAT_SCALAR_HC)
    cyc = itertools.cycle(itertools.product((True, False), ("relu", None)))
    for name, d in _sweep(tuple(GAT_VEC_HC), tuple(GAT_SCALAR_HC)):
        concat, act = next(cyc)
        H, C = hc[d]
        cases.append(GatCase(_cid("gat", name, f"H{H}C{C}", "cat" if concat else "mean", act), name, H, C, concat, act, 0.0))
    for p in (0.5, 0.3):
        for name, (H, C), concat in (("lengths", (3, 3), True), ("edge_empties", (1, 7), True), ("lengths", (3, 12), True),
                                     ("one_row", (2, 16), True), ("flat50", (3, 11), False), ("flat50", (4, 16), False)):
            cases.append(GatCase(_cid("gat", name, f"H{H}C{C}", "cat" if concat else "mean", "relu", f"p{p}"), name, H, C, concat, "relu", p))
    assert len({c.id for c in cases}) == len(cases)
    return cases


GAT_CASES = _gat_cases()


def gat_inputs(c):
    n_src, n_dst, ei = structures()[c.struct]
    rng = np.random.default_rng(hash_id(c.id))
    d = c.H * c.C
    width = d if c.concat else c.C
    relu = c.act == "relu"
    x = signed_rows(rng, n_src, d, c.C) if relu else randn(rng, n_src, d)
    b = signed_rows(rng, 1, width, c.C)[0] if relu else randn(rng, width)
    return dict(n_src=n_src, n_dst=n_dst, ei=torch.from_numpy(ei), x=x, al=logit_terms(rng, n_src, c.H, False),
                ar=logit_terms(rng, n_dst, c.H, True), b=b, G=randn(rng, n_dst, width))


def gat_reference(c, inp, mask):
    """``(y, {'gx', 'gal', 'gar', 'gb'}, logit margin, relu margin)`` from ``cegat_oracle.gat_hop``."""
    leaves = [inp[k].clone().requires_grad_(True) for k in ("x", "al", "ar", "b")]
    rep = {}
    y = cegat_oracle.gat_hop(leaves[0], leaves[1], leaves[2], inp["ei"], inp["n_dst"], c.H, 0.2, c.concat, leaves[3], c.act, mask, rep)
    (y * inp["G"]).sum().backward()
    with torch.no_grad():
        pre = cegat_oracle.gat_hop(inp["x"], inp["al"], inp["ar"], inp["ei"], inp["n_dst"], c.H, 0.2, c.concat, inp["b"])
    margin = float(pre.abs().min()) if c.act == "relu" else float("inf")
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in zip(("gx", "gal", "gar", "gb"), leaves)}
    return y.detach(), grads, rep["min_abs_logit"], margin


# ---- family 3: hattn_propagate (csrc/hattn.hip) ------------------------------------------------------------------------------------
HattnCase = namedtuple("HattnCase", "id struct H C concat act p p_attn")


def _hattn_cases():
    cases = []
    hc = dict(GAT_VEC_HC)
    hc.update(GAT_SCALAR_HC)
    cyc = itertools.cycle(itertools.product((True, False), ("relu", None, "elu"), (0.0, 0.5)))
    for name, d in _sweep(tuple(GAT_VEC_HC), tuple(GAT_SCALAR_HC)):
        concat, act, p_attn = next(cyc)
        H, C = hc[d]
        cases.append(HattnCase(_cid("hattn", name, f"H{H}C{C}", "cat" if concat else "mean", act, f"pa{p_attn}"), name, H, C, concat, act,
                               0.0, p_attn))
    for p in (0.5, 0.3):
        for name, (H, C), concat in (("lengths", (3, 3), True), ("edge_empties", (1, 7), True), ("lengths", (3, 12), True),
                                     ("flat50", (3, 11), False), ("flat50", (4, 16), False)):
            cases.append(HattnCase(_cid("hattn", name, f"H{H}C{C}", "cat" if concat else "mean", "relu", f"p{p}"), name, H, C, concat,
                                   "relu", p, p))
    for H, C in ((3, 129), (1, 131), (3, 132)):                          # 16 and 4 scalar packets per lane, 4 16-byte packets per lane
        cases.append(HattnCase(_cid("hattn", "lengths", f"H{H}C{C}", "cat", "elu", "packets"), "lengths", H, C, True, "elu", 0.0, 0.0))
    assert len({c.id for c in cases}) == len(cases)
    return cases


def hattn_packets(H, C):
    """csrc/hattn.hip geometry(): (VEC, packets per lane) of ``H`` heads of ``C`` channels on contiguous rows."""
    vec = 4 if C % 4 == 0 else 1
    hp = 1
    while hp < H:
        hp *= 2
    per, lh = (C + vec - 1) // vec, 1
    while lh < per and lh * hp < 64:
        lh *= 2
    need, npl = (per + lh - 1) // lh, 1
    while npl < need:
        npl *= 2
    return vec, npl


HATTN_CASES = _hattn_cases()


def hattn_inputs(c):
    """The structure read as (vertex, hyperedge) pairs: sources = vertices, targets = hyperedges.  Isolated vertices and empty
    hyperedges come with the structures; ``D`` / ``B`` are the layer's own (0 at an isolated vertex / empty hyperedge)."""
    n_v, n_e, ei = structures()[c.struct]
    ei = torch.from_numpy(ei)
    rng = np.random.default_rng(hash_id(c.id))
    d = c.H * c.C
    width = d if c.concat else c.C
    relu = c.act == "relu"
    z = signed_rows(rng, n_v, d, c.C) if relu else randn(rng, n_v, d)
    b = signed_rows(rng, 1, width, c.C)[0] if relu else randn(rng, width)
    D, B = hcha_attn_oracle.scales(ei, n_v, n_e, positive(rng, n_e))
    D, B = D.float().double(), B.float().double()
    return dict(n_v=n_v, n_e=n_e, ei=ei, z=z, av=logit_terms(rng, n_v, c.H, False), ae=logit_terms(rng, n_e, c.H, True), b=b, D=D, B=B,
                G=randn(rng, n_v, width))


def hattn_reference(c, inp, coef_mask, out_mask):
    """``(y, {'gz', 'gav', 'gae', 'gb'}, logit margin, relu margin)`` from ``hcha_attn_oracle.propagate``."""
    leaves = [inp[k].clone().requires_grad_(True) for k in ("z", "av", "ae", "b")]
    ei = inp["ei"]
    y = hcha_attn_oracle.propagate(leaves[0], leaves[1], leaves[2], ei, inp["n_e"], c.H, inp["D"], inp["B"], 0.2, c.concat, leaves[3],
                                   c.act, coef_mask, out_mask)
    (y * inp["G"]).sum().backward()
    with torch.no_grad():
        pre = hcha_attn_oracle.propagate(inp["z"], inp["av"], inp["ae"], ei, inp["n_e"], c.H, inp["D"], inp["B"], 0.2, c.concat, inp["b"],
                                         None, coef_mask, None)
        logit = inp["av"][ei[0]] + inp["ae"][ei[1]]
    margin = float(pre.abs().min()) if c.act == "relu" else float("inf")
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in zip(("gz", "gav", "gae", "gb"), leaves)}
    return y.detach(), grads, (float(logit.abs().min()) if logit.numel() else float("inf")), margin


# ---- family 4: unignn_hop, unigat_edge (csrc/unignn.hip), unigcn_hop (csrc/unigcn.hip) --------------------------------------------------
# The structures read as (vertex, hyperedge) pairs; the E->V hops gather hyperedge rows into vertex rows.  The fused launches are built
# for 16-byte rows up to 512 columns; every other width takes the documented unfused composition (``ops.*_supported`` says which).
import unigcnii_oracle  # noqa: E402
import unignn_oracle  # noqa: E402

UnignnCase = namedtuple("UnignnCase", "id struct d use_norm has_s self_term act p variant")
UnigatCase = namedtuple("UnigatCase", "id struct H C has_s variant")
UnigcnCase = namedtuple("UnigcnCase", "id struct d use_norm variant")
UNI_SHORT_ROW_MESSAGE = "the short-row variant needs"
UNI_VARIANT_ERRORS = [("flat50", 260), ("lengths", 512)]


def uni_fused(d, C=None):
    """What ``ops.unignn_hop_supported`` / ``unigcn_hop_supported`` / ``unignn_v2e_att_supported`` say for contiguous fp32 operands."""
    return d % 4 == 0 and d <= 512 and (C is None or C % 4 == 0)


def _uni_variant(variant, d):
    return 1 if (variant == 2 and d > 256) else variant               # (a forced 2 above 256 columns is refused: UNI_VARIANT_ERRORS)


def _unignn_cases():
    cases = []
    cyc = itertools.cycle(itertools.product((True, False), (True, False), ("none", "float", "tensor"), (None, "relu"), (2, None, 1)))
    for name, d in _sweep(VEC_WIDTHS, SCALAR_WIDTHS):
        use_norm, has_s, self_term, act, variant = next(cyc)
        variant = _uni_variant(variant, d)
        cases.append(UnignnCase(_cid("unignn", name, d, "norm" if use_norm else "plain", "s" if has_s else "", self_term, act, f"v{variant}"),
                                name, d, use_norm, has_s, self_term, act, 0.0, variant))
    # the row norm on rows that are exactly zero (isolated vertices, no self term), through both kernels and the composition
    for name, d, variant in (("edge_empties", 12, 2), ("edge_empties", 36, 1), ("one_col", 68, 2), ("empty", 132, 1), ("wide", 260, 1),
                             ("edge_empties", 7, None), ("dups", 64, 2), ("one_col", 256, 2)):
        cases.append(UnignnCase(_cid("unignn", name, d, "norm", "s", "none", "zero-rows", f"v{variant}"), name, d, True, True, "none", None, 0.0,
                                variant))
    for name in ("flat50", "lengths"):                                    # the short-row kernel's row tail at every lane-group width
        for d in (12, 36, 68, 132):
            cases.append(UnignnCase(_cid("unignn", name, d, "norm", "s", "float", "relu", "v2", "flat"), name, d, True, True, "float", "relu",
                                    0.0, 2))
    for p in (0.5, 0.3):
        for name, d, variant in (("lengths", 7, None), ("flat50", 33, None), ("flat50", 36, 2), ("lengths", 260, 1), ("edge_empties", 12, 2)):
            cases.append(UnignnCase(_cid("unignn", name, d, "norm", "s", "tensor", "relu", f"p{p}", f"v{variant}"), name, d, True, True, "tensor",
                                    "relu", p, variant))
    assert len({c.id for c in cases}) == len(cases)
    return cases


def _unigat_cases():
    cases = []
    hc = dict(GAT_VEC_HC)
    hc.update(GAT_SCALAR_HC)
    cyc = itertools.cycle(itertools.product((True, False), (None, 2, 1)))
    for name, d in _sweep(tuple(GAT_VEC_HC), tuple(GAT_SCALAR_HC)):
        has_s, variant = next(cyc)
        H, C = hc[d]
        variant = _uni_variant(variant, d)
        cases.append(UnigatCase(_cid("unigat", name, f"H{H}C{C}", "s" if has_s else "", f"v{variant}"), name, H, C, has_s, variant))
    for name in ("flat50", "lengths"):                                    # the short-row kernel's head reductions at every lane-group width
        for H, C in ((3, 4), (3, 12), (1, 68), (3, 44), (4, 64)):
            cases.append(UnigatCase(_cid("unigat", name, f"H{H}C{C}", "s", "v2", "flat"), name, H, C, True, 2))
    assert len({c.id for c in cases}) == len(cases)
    return cases


def _unigcn_cases():
    cases = []
    cyc = itertools.cycle(itertools.product((True, False), (1, None, 2)))
    for name, d in _sweep(VEC_WIDTHS, SCALAR_WIDTHS):
        use_norm, variant = next(cyc)
        variant = _uni_variant(variant, d)
        cases.append(UnigcnCase(_cid("unigcn", name, d, "norm" if use_norm else "plain", f"v{variant}"), name, d, use_norm, variant))
    for name in ("flat50", "lengths", "edge_empties"):
        for d in (12, 36, 68, 132):
            cases.append(UnigcnCase(_cid("unigcn", name, d, "norm", "v2", "flat"), name, d, True, 2))
    assert len({c.id for c in cases}) == len(cases)
    return cases


UNIGNN_CASES, UNIGAT_CASES, UNIGCN_CASES = _unignn_cases(), _unigat_cases(), _unigcn_cases()
UNIGNN_C = 1.25                                                           # the tensor self-term coefficient


def unignn_inputs(c):
    n_v, n_e, ei = structures()[c.struct]
    rng = np.random.default_rng(hash_id(c.id))
    relu = c.act == "relu"
    xe = signed_rows(rng, n_e, c.d) if relu else randn(rng, n_e, c.d)
    xs = signed_rows(rng, n_v, c.d) if relu else randn(rng, n_v, c.d)
    s = positive(rng, n_v) + 0.5 if c.has_s else None                     # [1, 2): s * |sum| keeps the 0.25 of one term
    return dict(n_v=n_v, n_e=n_e, ei=torch.from_numpy(ei), xe=xe, xs=xs if c.self_term != "none" else None, s=s, G=randn(rng, n_v, c.d))


def unignn_reference(c, inp, mask):
    """``(y, {'gxe', 'gxs', 'gc'}, t or None, relu margin)`` from ``unignn_oracle.hop``.  The margin is taken on the row BEFORE the
    norm (``t`` is a positive scale: it moves no sign) and over the rows that hold anything: a vertex without incidence and without
    self term is an exact zero row on both sides, where relu and its derivative are 0 in fp32 and in float64 alike."""
    V, E = inp["ei"][0], inp["ei"][1]
    xe = inp["xe"].clone().requires_grad_(True)
    xs = inp["xs"].clone().requires_grad_(True) if inp["xs"] is not None else None
    c64 = torch.tensor([UNIGNN_C], dtype=D64, requires_grad=True)
    coef = c64 if c.self_term == "tensor" else 1.0
    rep = {}
    y = unignn_oracle.hop(xe, V, E, inp["n_v"], s=inp["s"], xs=xs, c=coef, use_norm=c.use_norm, act=c.act, mask=mask, report=rep)
    (y * inp["G"]).sum().backward()
    margin = float("inf")
    if c.act == "relu":
        with torch.no_grad():
            pre = unignn_oracle.hop(inp["xe"], V, E, inp["n_v"], s=inp["s"], xs=inp["xs"], c=float(coef))
        rows = torch.ones(inp["n_v"], dtype=torch.bool) if xs is not None else torch.bincount(V, minlength=inp["n_v"]) > 0
        assert bool((pre[~rows] == 0).all())
        margin = float(pre[rows].abs().min()) if bool(rows.any()) else float("inf")
    grads = dict(gxe=xe.grad if xe.grad is not None else torch.zeros_like(xe), gxs=None if xs is None else xs.grad,
                 gc=c64.grad if c.self_term == "tensor" else None)
    return y.detach(), grads, rep.get("t"), margin


def unigat_inputs(c):
    n_v, n_e, ei = structures()[c.struct]
    rng = np.random.default_rng(hash_id(c.id))
    d = c.H * c.C
    return dict(n_v=n_v, n_e=n_e, ei=torch.from_numpy(ei), x=randn(rng, n_v, d), att=randn(rng, c.H, c.C),
                s=positive(rng, n_e) if c.has_s else None, G=randn(rng, n_e, d), Ga=randn(rng, n_e, c.H))


def unigat_reference(c, inp):
    """``(xe, ae, {'gx', 'gatt'})`` from ``unignn_oracle.edge_logits`` under ``(xe * G).sum() + (ae * Ga).sum()``."""
    x = inp["x"].clone().requires_grad_(True)
    att = inp["att"].clone().requires_grad_(True)
    xe, ae = unignn_oracle.edge_logits(x, inp["ei"][0], inp["ei"][1], inp["n_e"], inp["s"], att, c.H)
    ((xe * inp["G"]).sum() + (ae * inp["Ga"]).sum()).backward()
    return xe.detach(), ae.detach(), dict(gx=x.grad if x.grad is not None else torch.zeros_like(x), gatt=att.grad)


UNIGCN_ALPHA = 0.1


def unigcn_inputs(c):
    n_v, n_e, ei = structures()[c.struct]
    rng = np.random.default_rng(hash_id(c.id))
    return dict(n_v=n_v, n_e=n_e, ei=torch.from_numpy(ei), xe=randn(rng, n_e, c.d), x0=randn(rng, n_v, c.d), degV=positive(rng, n_v),
                G=randn(rng, n_v, c.d))


def unigcn_reference(c, inp):
    """``(xi, {'gxe', 'gx0'})`` from ``unigcnii_oracle.hop``."""
    xe = inp["xe"].clone().requires_grad_(True)
    x0 = inp["x0"].clone().requires_grad_(True)
    xi = unigcnii_oracle.hop(xe, x0, inp["ei"][0], inp["ei"][1], inp["degV"], UNIGCN_ALPHA, c.use_norm)
    (xi * inp["G"]).sum().backward()
    return xi.detach(), dict(gxe=xe.grad if xe.grad is not None else torch.zeros_like(xe), gx0=x0.grad)


# ---- family 5: han_gat_propagate, han_block_propagate (csrc/han.hip) ----------------------------------------------------------------
# A ``han.MetapathGraph`` is a multigraph over ONE node set in which every node has an incoming edge: a structure is read over
# ``n = max(n_src, n_dst)`` nodes and a self-loop is ADDED at every node without an incoming edge (DGL's add_self_loop, as
# ``han.metapath_graphs`` does) -- so the runs of empty rows become runs of one-edge rows here.  A ``han_sampling.Block`` keeps the
# rectangle (its targets are its first source nodes, ``n_dst <= n_src``; a sampled block carries every target's self-loop, added here
# the same way); ``n_dst > n_src`` is the constructor's error.
import han_oracle  # noqa: E402
import han_sampling_oracle  # noqa: E402

HanCase = namedtuple("HanCase", "id struct H C block p")
HAN_BLOCK_ERROR = "a block's targets are its first source nodes"


def han_edges(name, block):
    """``(n_src, n_dst, src, dst)`` int64 tensors: the structure's edges plus a self-loop at every target without an incoming edge."""
    n_src, n_dst, ei = structures()[name]
    if not block:
        n_src = n_dst = max(n_src, n_dst)
    lonely = np.flatnonzero(np.bincount(ei[1], minlength=n_dst) == 0)
    ei = np.concatenate([ei, np.stack([lonely, lonely])], axis=1)
    return n_src, n_dst, torch.from_numpy(ei[0].copy()), torch.from_numpy(ei[1].copy())


def han_block_ok(name):
    n_src, n_dst, _ = structures()[name]
    return n_dst <= n_src


def _han_cases():
    cases = []
    hc = dict(GAT_VEC_HC)
    hc.update(GAT_SCALAR_HC)
    for name, d in _sweep(tuple(GAT_VEC_HC), tuple(GAT_SCALAR_HC)):
        H, C = hc[d]
        cases.append(HanCase(_cid("han", name, f"H{H}C{C}"), name, H, C, False, 0.0))
    blocks = [n for n in structures() if han_block_ok(n)]
    for i, name in enumerate(blocks):
        for d in (tuple(GAT_VEC_HC)[(3 * i + 1) % 11], tuple(GAT_SCALAR_HC)[(3 * i + 1) % 8]):
            H, C = hc[d]
            cases.append(HanCase(_cid("hanblock", name, f"H{H}C{C}"), name, H, C, True, 0.0))
    for p in (0.5, 0.3):
        for name, (H, C), block in (("lengths", (3, 3), False), ("edge_empties", (1, 7), False), ("lengths", (3, 12), False),
                                    ("dups", (4, 16), False), ("one_row", (3, 11), True), ("wide", (2, 16), True)):
            cases.append(HanCase(_cid("hanblock" if block else "han", name, f"H{H}C{C}", f"p{p}"), name, H, C, block, p))
    assert len({c.id for c in cases}) == len(cases)
    return cases


HAN_CASES = _han_cases()
HAN_BLOCK_ERRORS = [n for n in structures() if not han_block_ok(n)]


def han_inputs(c):
    n_src, n_dst, src, dst = han_edges(c.struct, c.block)
    rng = np.random.default_rng(hash_id(c.id))
    d = c.H * c.C
    return dict(n_src=n_src, n_dst=n_dst, src=src, dst=dst, x=randn(rng, n_src, d), el=logit_terms(rng, n_src, c.H, False),
                er=logit_terms(rng, n_dst, c.H, True), b=randn(rng, d), G=randn(rng, n_dst, d))


# The one case whose gradient needs more than the family rule.  With every edge leaving ONE source (``one_col``) and every target's
# softmax running over that edge and its own self-loop, the source's ``gel[s, h] = sum_j a_j lrelu'_j (<x_s, g_tj> - delta_tj)`` sums
# 1500 terms of magnitude O(1) that cancel to O(1e-15) in float64 -- the family rule's scale, max |want|, is then no scale at all.
# The kernel forms the sum as the difference of two accumulated sums (csrc/han.hip: no per-incidence dot product), so the project's
# own error model of a sum applies (tests/test_gpu_ce_implicit.py): an fp32 sum of m terms is within m * 2^-23 * sum |terms| (twice the
# first-order worst case).  ``han_gel_slack`` evaluates that from the float64 reference: per (source, head), m = (edges leaving the
# source) + C and sum |terms| = sum_j a_j lrelu'_j (sum_c |x_s g_tj| + |delta_tj|).  Observed on the MI355X: |diff| 1.3e-4 against
# want 3.7e-15 (family tolerance 1e-4); the slack is ~1e0 at the hub source and ~1e-5 elsewhere.
HAN_GEL_SLACK = ("han-one_col-H3C11",)


def han_gel_slack(c, inp, edge_keep):
    """float64 [n_src, H]: ``m * 2^-23 * sum |terms|`` of ``gel`` (see HAN_GEL_SLACK), from the reference's quantities alone."""
    H, C, src, dst, n_src, n_dst = c.H, c.C, inp["src"], inp["dst"], inp["n_src"], inp["n_dst"]
    x = inp["x"].view(n_src, H, C)
    pre = inp["el"][src] + inp["er"][dst]
    e = torch.nn.functional.leaky_relu(pre, 0.2)
    mx = torch.full((n_dst, H), -float("inf"), dtype=D64).scatter_reduce(0, dst.view(-1, 1).expand(-1, H), e, "amax", include_self=True)
    ex = torch.exp(e - mx[dst])
    a = ex / torch.zeros((n_dst, H), dtype=D64).index_add(0, dst, ex)[dst]
    a = a if edge_keep is None else a * edge_keep
    rst = torch.zeros((n_dst, H, C), dtype=D64).index_add(0, dst, x[src] * a.unsqueeze(-1))
    z = rst + inp["b"].view(1, H, C)
    g = inp["G"].view(n_dst, H, C) * torch.where(z > 0, torch.ones_like(z), torch.exp(z))          # elu'
    delta = (rst * g).sum(-1)
    terms = a * torch.where(pre > 0, 1.0, 0.2) * ((x[src].abs() * g[dst].abs()).sum(-1) + delta[dst].abs())
    A = torch.zeros((n_src, H), dtype=D64).index_add(0, src, terms)
    m = torch.bincount(src, minlength=n_src).double() + C
    return m.unsqueeze(1) * 2.0 ** -23 * A


def han_reference(c, inp, edge_keep):
    """``(y, {'gx', 'gel', 'ger', 'gb'}, logit margin)`` from ``han_oracle.gat_hop`` (full graph) or ``han_sampling_oracle.gat_hop``
    (block); the activation is elu: no kink but the logit's."""
    leaves = [inp[k].clone().requires_grad_(True) for k in ("x", "el", "er", "b")]
    rep = []
    if c.block:
        y = han_sampling_oracle.gat_hop(inp["src"], inp["dst"], inp["n_src"], inp["n_dst"], leaves[0], leaves[1], leaves[2], leaves[3],
                                        edge_keep, rep)
    else:
        y = han_oracle.gat_hop(inp["src"], inp["dst"], inp["n_dst"], leaves[0], leaves[1], leaves[2], leaves[3], edge_keep, rep)
    (y * inp["G"]).sum().backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in zip(("gx", "gel", "ger", "gb"), leaves)}
    return y.detach(), grads, rep[0]


# ---- family 6: clique_propagate (csrc/scan.hip) --------------------------------------------------------------------------------------
# The structures read as V->E lists (row 0 vertices, row 1 hyperedges); the reference is tests/ce_oracle.py over the EXPLICIT expansion
# (clique_expansion + gcn_norm as a dense normalised adjacency).  A list without a hyperedge of two members has no expansion:
# ``baselines.ImplicitCEGraph`` raises ``gcn_norm``'s error for it.
import ce_oracle  # noqa: E402

CliqueCase = namedtuple("CliqueCase", "id struct d act p")
CLIQUE_EMPTY_MESSAGE = "gcn_norm: expected a non-empty"
_CE_ADJ = {}


def clique_adjacency(name, T=LOO_LONG_T):
    """float64 [n_v, n_v] ``M`` with ``y = M @ x`` the GCN hop over the explicit clique expansion, or None when there is no pair."""
    if (name, T) not in _CE_ADJ:
        n_v, _, ei = structures(T)[name]
        pairs, mult = ce_oracle.clique_expansion(torch.from_numpy(ei))
        M = None
        if pairs.numel():
            oei, ow = ce_oracle.gcn_norm(pairs, mult)
            M = torch.zeros(n_v, n_v, dtype=D64).index_put_((oei[1], oei[0]), ow, accumulate=True)
        _CE_ADJ[(name, T)] = M
    return _CE_ADJ[(name, T)]


def _clique_cases():
    cases = []
    names = [n for n in structures() if n not in CLIQUE_NO_PAIR]
    cyc = itertools.cycle((None, "relu", "elu"))
    pairs = []
    for i, name in enumerate(names):
        pairs += [(name, VEC_WIDTHS[(2 * i) % 11]), (name, SCALAR_WIDTHS[(2 * i) % 8])]
    for name in ("edge_empties", "lengths"):
        pairs += [(name, d) for d in VEC_WIDTHS + SCALAR_WIDTHS if (name, d) not in pairs]
    for name, d in pairs:
        act = next(cyc)
        cases.append(CliqueCase(_cid("clique", name, d, act), name, d, act, 0.0))
    for p in (0.5, 0.3):
        for name, d in (("lengths", 7), ("flat50", 33), ("lengths", 36), ("edge_empties", 260)):
            cases.append(CliqueCase(_cid("clique", name, d, "relu", f"p{p}"), name, d, "relu", p))
    assert len({c.id for c in cases}) == len(cases)
    return cases


CLIQUE_NO_PAIR = ("empty", "single", "one_col")                           # no hyperedge with two members: the constructor's error
CLIQUE_CASES = _clique_cases()


def clique_inputs(c):
    n_v, n_e, ei = structures(LOO_LONG_T)[c.struct]
    rng = np.random.default_rng(hash_id(c.id))
    relu = c.act == "relu"
    return dict(n_v=n_v, ei=torch.from_numpy(ei), x=signed_rows(rng, n_v, c.d) if relu else randn(rng, n_v, c.d),
                b=signed_rows(rng, 1, c.d)[0] if relu else randn(rng, c.d), G=randn(rng, n_v, c.d))


def clique_reference(c, inp, mask):
    """``(y, {'gx', 'gb'}, relu margin)``: the normalised adjacency is non-negative, so the sign construction holds."""
    M = clique_adjacency(c.struct)
    x, b = inp["x"].clone().requires_grad_(True), inp["b"].clone().requires_grad_(True)
    pre = M @ x + b
    y = torch.relu(pre) if c.act == "relu" else torch.nn.functional.elu(pre) if c.act == "elu" else pre
    y = y * mask if mask is not None else y
    (y * inp["G"]).sum().backward()
    assert float(M.min()) >= 0.0
    return y.detach(), dict(gx=x.grad, gb=b.grad), (float(pre.detach().abs().min()) if c.act == "relu" else float("inf"))


# ---- family 7: deepsets_aggregate_exclude_self (csrc/loo.hip), pma_aggregate_exclude_self (csrc/loo_softmax.hip) ------------------------
# The structures read as V->E lists, sorted by vertex, hyperedge ids behind the vertex ids (as tests/test_gpu_exclude_self*.py build
# theirs); ``lengths`` is built around ``ops.loo_long_threshold()``.  The reference is the float64 product with the dense incidence of
# the EXPANDED list (``preprocessing.expand_edge_index``), with the expansion's own weights.  A repeated (vertex, hyperedge) pair makes
# the expansion ill-defined: ``LeaveOneOutIncidence`` refuses it.  A width that is no multiple of 4 is not built and has no fallback.
LooCase = namedtuple("LooCase", "id struct kind H C aggr normtype")
LOO_DUPLICATE_MESSAGE = "duplicate \\(vertex, hyperedge\\) incidences"
LOO_DUPLICATES = ("one_row", "one_col", "dups")
LOO_UNBUILT = [("ds", 1, 3), ("ds", 1, 33), ("pma", 3, 4), ("pma", 1, 7)]   # (kind, heads, channels): 'is not built'
LOO_PMA_HC = OrderedDict([(4, (1, 4)), (12, (1, 12)), (32, (2, 16)), (36, (1, 36)), (64, (4, 16)), (68, (1, 68)), (128, (8, 16)),
                          (132, (1, 132)), (256, (4, 64)), (260, (1, 260)), (512, (8, 64))])
U23 = 2.0 ** -23


def loo_list(name):
    """``(n_v, n_e, ei)``: the structure's pairs sorted by (vertex, hyperedge), hyperedge ids from ``n_v``."""
    n_v, n_e, ei = structures(LOO_LONG_T)[name]
    ei = torch.from_numpy(ei)
    ei = ei[:, torch.argsort(ei[0] * max(n_e, 1) + ei[1])]
    return n_v, n_e, torch.stack([ei[0], ei[1] + n_v])


def _loo_cases():
    cases = []
    names = [n for n in structures() if n not in LOO_DUPLICATES]
    combos = itertools.cycle(itertools.product(("add", "mean"), ("all_one", "deg_half_sym")))
    pairs = []
    for i, name in enumerate(names):
        pairs += [(name, VEC_WIDTHS[(3 * i) % 11]), (name, VEC_WIDTHS[(3 * i + 5) % 11])]
    for name in ("edge_empties", "lengths"):
        pairs += [(name, d) for d in VEC_WIDTHS if (name, d) not in pairs]
    for name, d in pairs:
        aggr, normtype = next(combos)
        cases.append(LooCase(_cid("loo", name, d, aggr, normtype), name, "ds", 1, d, aggr, normtype))
        H, C = LOO_PMA_HC[d]
        if name == "wide" and H > 2:                                      # (the dense float64 softmax is [nnz, n_v, H]: keep it small)
            H, C = 1, d
        cases.append(LooCase(_cid("loopma", name, f"H{H}C{C}"), name, "pma", H, C, None, None))
    assert len({c.id for c in cases}) == len(cases)
    return cases


LOO_CASES = _loo_cases()
_LOO_REF = {}


def loo_expansion(name):
    """Once per structure: the expanded incidence as index lists (``ev`` vertex, ``ep`` expanded hyperedge = position), sizes, degrees."""
    if name not in _LOO_REF:
        from types import SimpleNamespace
        from allset_amd import preprocessing as P
        n_v, n_e, ei = loo_list(name)
        nnz = ei.shape[1]
        n_dst = int(ei[0].max()) + 1 if nnz else 0
        if nnz:
            data = P.expand_edge_index(SimpleNamespace(edge_index=ei.clone(), n_x=[n_v], num_hyperedges=[n_e]))
            ev, ep = data.edge_index[0], data.edge_index[1] - n_v
            assert int(ep.max()) + 1 == nnz
        else:
            ev = ep = torch.zeros(0, dtype=torch.int64)
        _LOO_REF[name] = dict(n_v=n_v, n_e=n_e, ei=ei, nnz=nnz, n_dst=n_dst, ev=ev, ep=ep, size=torch.bincount(ep, minlength=nnz).double(),
                              deg=torch.bincount(ev, minlength=n_v).double())
    return _LOO_REF[name]


def loo_matrices(name, aggr, normtype):
    """``(A [nnz, n_v], B [n_dst, nnz], terms_e [nnz, 1], terms_v [n_v, 1])`` float64: V->E is ``A @ x``, E->V is ``B @ y``; ``terms``
    the number of products an output sums, the error model's m (tests/test_gpu_exclude_self.py)."""
    r = loo_expansion(name)
    ev, ep, size, deg = r["ev"], r["ep"], r["size"], r["deg"]
    w = torch.ones(ev.numel(), dtype=D64) if normtype == "all_one" else deg[ev].pow(-0.5) * size[ep].pow(-0.5)
    A = torch.zeros(r["nnz"], r["n_v"], dtype=D64)
    A[ep, ev] = w / size[ep] if aggr == "mean" else w
    B = torch.zeros(r["n_dst"], r["nnz"], dtype=D64)
    B[ev, ep] = w / deg[ev] if aggr == "mean" else w
    kmax = torch.zeros(r["n_v"], dtype=D64).index_reduce_(0, ev, size[ep], "amax") if ev.numel() else torch.zeros(r["n_v"], dtype=D64)
    return A, B, size.unsqueeze(1), (deg + kmax).unsqueeze(1)


def loo_inputs(c):
    r = loo_expansion(c.struct)
    rng = np.random.default_rng(hash_id(c.id))
    d = c.H * c.C
    return dict(x=randn(rng, r["n_v"], d), y=randn(rng, r["nnz"], d), G_e=randn(rng, r["nnz"], d), G_v=randn(rng, r["n_dst"], d),
                ax=logit_terms(rng, r["n_v"], c.H, True), ay=logit_terms(rng, r["nnz"], c.H, True))


def loo_bound_check(got, M, inp, terms, what):
    """The exclude-self family's own rule: ``|got - M @ inp| <= (terms + 8) * 2^-23 * (|M| @ |inp|)`` per element."""
    got = got.detach().cpu().double()
    ref = M @ inp
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} against {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    bound = (terms[:ref.shape[0]] + 8) * U23 * (M.abs() @ inp.abs())
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max err / bound = {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: max err / bound = {worst}"


def dense_pma64(V, alpha, mask, H, slope=0.2):
    """Float64 softmax pooling with the dense incidence ``mask`` [targets, sources] (tests/test_gpu_exclude_self_pma.py)."""
    a = torch.nn.functional.leaky_relu(alpha, slope)
    has = mask.any(dim=1, keepdim=True)
    logits = torch.where((mask | ~has).unsqueeze(2), a.unsqueeze(0), torch.full((), -float("inf"), dtype=D64))
    w = torch.softmax(logits, dim=1) * has.unsqueeze(2)
    return torch.einsum("tsh,shc->thc", w, V.view(V.shape[0], H, -1)).reshape(mask.shape[0], -1)


def loo_pma_reference(c, inp):
    """Per direction ``(out, gV, galpha)`` from the dense float64 softmax over the expanded incidence."""
    r = loo_expansion(c.struct)
    A = torch.zeros(r["nnz"], r["n_v"], dtype=torch.bool)
    A[r["ep"], r["ev"]] = True
    B = A.t()[:r["n_dst"]].contiguous()
    out = {}
    for direction, V, al, G, mask in (("v2e", inp["x"], inp["ax"], inp["G_e"], A), ("e2v", inp["y"], inp["ay"], inp["G_v"], B)):
        if mask.numel() == 0:
            out[direction] = (torch.zeros(mask.shape[0], V.shape[1], dtype=D64), torch.zeros_like(V), torch.zeros_like(al))
            continue
        V64, a64 = V.clone().requires_grad_(True), al.clone().requires_grad_(True)
        ref = dense_pma64(V64, a64, mask, c.H)
        gV, ga = torch.autograd.grad(ref, (V64, a64), G)
        out[direction] = (ref.detach(), gV, ga)
    return out


def units(got, ref):
    """Worst error in units of the PMA kernels' own tolerance, ``1e-4 + 1e-4 * |reference|`` (tests/test_gpu_ops.py ATOL / RTOL)."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, f"shape {tuple(got.shape)} against {tuple(ref.shape)}"
    return float(((got - ref).abs() / (1e-4 + 1e-4 * ref.abs())).max()) if ref.numel() else 0.0


# ---- the short-row kernels of csrc/segreduce.hip and csrc/pma.hip (ops.segreduce / pma_fwd / pma_bwd_src with variant=2) ---------------
# tests/test_gpu_flat_walk.py: every structure at every width the kernels build (one column chunk, d <= 256), against the float64
# operator seam of oracle/allset_oracle.py that tests/test_gpu_ops.py holds these kernels to.
FLAT_WIDTHS = tuple(d for d in VEC_WIDTHS if d <= 256)
FLAT_PMA_HC = OrderedDict((d, hc) for d, hc in GAT_VEC_HC.items() if d <= 256)
FLAT_SPLIT_STRUCT = "lengths"                     # long and short rows in one CSR: ops.size_split at CSR_LONG_T cuts off the T + 1 row


def flat_segreduce_inputs(name, d):
    n_src, n_dst, ei = structures()[name]
    rng = np.random.default_rng(hash_id(_cid("flat-seg", name, d)))
    return dict(n_src=n_src, n_dst=n_dst, ei=torch.from_numpy(ei), x=randn(rng, n_src, d), w=positive(rng, ei.shape[1]))


def flat_segreduce_reference(inp, x, aggr, weighted):
    """``oracle.deepsets_aggregate`` in float64, padded to ``n_dst`` rows (the scatter stops at the last row that received anything;
    without any incidence every row is 0)."""
    from oracle import allset_oracle
    nnz = inp["ei"].shape[1]
    if nnz == 0:
        return torch.zeros(inp["n_dst"], x.shape[1], dtype=D64)
    out = allset_oracle.deepsets_aggregate(x, inp["ei"], inp["w"] if weighted else torch.ones(nnz, dtype=D64), aggr)
    return torch.cat([out, out.new_zeros(inp["n_dst"] - out.shape[0], x.shape[1])])


def flat_pma_inputs(name, H, C, transposed):
    """``transposed``: the structure's target rows become the SOURCES (the rows of the backward's transposed CSR)."""
    n_src, n_dst, ei = structures()[name]
    if transposed:
        n_src, n_dst, ei = n_dst, n_src, ei[::-1].copy()
    rng = np.random.default_rng(hash_id(_cid("flat-pma", name, H, C, transposed)))
    return dict(n_src=n_src, n_dst=n_dst, ei=torch.from_numpy(ei), H=H, C=C, V=randn(rng, n_src, H * C),
                alpha=logit_terms(rng, n_src, H, True), G=randn(rng, n_dst, H * C))


def flat_pma_reference(inp):
    """``(out, m, l, gV, galpha)``: ``oracle.pma_aggregate`` in float64 and its autograd under ``(out * G).sum()``; m and l are the two
    intermediates of ``oracle.segment_softmax`` (the segment max, 0 for a row that receives nothing, and the segment sum of
    exp(a - max)).  Without any incidence every output is 0 (the scatter's rule)."""
    from oracle import allset_oracle
    n_s, n_t, H, C, ei = inp["n_src"], inp["n_dst"], inp["H"], inp["C"], inp["ei"]
    if ei.shape[1] == 0:
        return (torch.zeros(n_t, H * C, dtype=D64), torch.zeros(n_t, H, dtype=D64), torch.zeros(n_t, H, dtype=D64),
                torch.zeros(n_s, H * C, dtype=D64), torch.zeros(n_s, H, dtype=D64))
    V, alpha = inp["V"].clone().requires_grad_(True), inp["alpha"].clone().requires_grad_(True)
    out, _ = allset_oracle.pma_aggregate(V.view(n_s, H, C), alpha, ei, 0.2)
    out = torch.cat([out, out.new_zeros(n_t - out.shape[0], H, C)]).reshape(n_t, H * C)
    gV, ga = torch.autograd.grad(out, (V, alpha), inp["G"])
    a = torch.nn.functional.leaky_relu(inp["alpha"].index_select(0, ei[0]), 0.2)
    m = allset_oracle.scatter(a, ei[1], n_t, "max")
    l = allset_oracle.scatter((a - m.index_select(0, ei[1])).exp(), ei[1], n_t, "sum")
    return out.detach(), m, l, gV, ga


# The one structure whose logit gradient cannot be held to the family rule's scale -- the backward's ``one_col`` (HAN_GEL_SLACK above):
# with the structure's rows as SOURCE rows, ``one_row`` has every incidence leaving ONE source, and every target's softmax runs over
# copies of that source alone, so ``galpha[s, h] = lrelu'(alpha_s) * sum_j p_j (<V_s, g_tj> - delta_tj)`` sums 1500 terms of magnitude
# O(1) that cancel to exactly 0 whatever the inputs -- max |want| is no scale at all.  pma_bwd_src_{,flat_}kernel form it as the
# difference of two accumulated fp32 sums (S - D, no per-incidence dot product), so what is left is those sums' rounding error.  Its
# allowance is the probabilistic bound of an m-term sum in precision u, ``sqrt(m) * u * sum |terms|`` (Higham & Mary 2019, lambda = 1;
# the worst-case ``m * u`` form that HAN_GEL_SLACK uses would be ~0.5 here and check nothing), with u = 2^-24, m = (incidences of the
# source) + C and sum |terms| = lrelu' * sum_j p_j (sum_c |V_s g_tj| + |delta_tj|), all from the float64 reference: 1e-3 .. 4e-2 at the
# hub source over the nine widths, where ONE dropped or doubled incidence moves galpha by p_j |delta_tj| ~ 0.05 .. 1 (host file).  Observed on the
# MI355X (parent's library and this one alike): |diff| 1.5e-4 against want 0 at d = 32.
FLAT_GALPHA_SLACK = ("one_row",)


def flat_pma_galpha_slack(inp):
    """float64 [n_src, H]: ``sqrt(m) * 2^-24 * sum |terms|`` of ``galpha`` (see FLAT_GALPHA_SLACK)."""
    from oracle import allset_oracle
    n_s, n_t, H, C, (src, dst) = inp["n_src"], inp["n_dst"], inp["H"], inp["C"], inp["ei"]
    V, G = inp["V"].view(n_s, H, C), inp["G"].view(n_t, H, C)
    p = allset_oracle.segment_softmax(torch.nn.functional.leaky_relu(inp["alpha"][src], 0.2), dst, n_t)
    delta = (allset_oracle.scatter(V[src] * p.unsqueeze(-1), dst, n_t, "sum") * G).sum(-1)
    terms = p * torch.where(inp["alpha"][src] > 0, 1.0, 0.2) * ((V[src].abs() * G[dst].abs()).sum(-1) + delta[dst].abs())
    m = torch.bincount(src, minlength=n_s).double() + C
    return m.sqrt().unsqueeze(1) * 2.0 ** -24 * allset_oracle.scatter(terms, src, n_s, "sum")
