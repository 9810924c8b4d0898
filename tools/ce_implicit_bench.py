"""CEGCN's GCN hop without the clique expansion (csrc/scan.hip) against the explicit path (ConstructV2V + gcn_norm,
allset_hconv_fwd_w), in one process.

Shapes: ``fixed16`` -- tools/ce_bench.py's: 1M vertices, 1M hyperedges of 16 members (drawn with replacement, as there), C = 128; and
``zipf4096`` -- 1M x 1M, Zipf sizes of mean 16 capped at 4096 (``synthetic.random_hypergraph(dist='zipf')``), where the explicit arm runs
only if its pair count stays below ``--pair-limit``.

Per shape: the forward hop (bias + relu + dropout 0.5 fused) and the backward hop (the transposed gather / the suffix scan + collect) of
both arms as hipEvent times -- the protocol of tools/exclude_self_ablation.py: the arms ALTERNATE inside the process, ``--repeats``
blocks of ``--iters`` event-timed calls each, a block's value its median; reported: the median over the blocks and their min / max --
the one-time graph build of both arms (hipEvents around the whole build, ``--build-repeats`` times, alternating), and each new launch on
its own through ``ops.KernelTimer`` with its algorithmic bytes as a fraction of 8 TB/s.

    python tools/ce_implicit_bench.py [--shapes fixed16,zipf4096] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import ops  # noqa: E402
from allset_amd.baselines import CEGraph, ImplicitCEGraph  # noqa: E402
from allset_amd.preprocessing import ConstructV2V, ConstructV2V_implicit, norm_contruction  # noqa: E402
from allset_amd.synthetic import random_hypergraph  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _block(fn, iters):
    return statistics.median(_event_ms(fn)[0] for _ in range(iters))


def _stat(ms):
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), blocks=ms)


def _edge_list(shape, n):
    if shape == "fixed16":
        g = torch.Generator(device=DEV).manual_seed(0)
        v = torch.randint(0, n, (n * 16,), device=DEV, generator=g)
        e = torch.arange(n, device=DEV).repeat_interleave(16)
        return torch.stack([v, e + n])
    return random_hypergraph(n, n, degree=16, seed=0, device=DEV, dist="zipf", max_degree=4096, e_base=n).edge_index


def measure(shape, n, d, repeats, iters, build_repeats, pair_limit):
    ei = _edge_list(shape, n)
    sizes = torch.bincount(ei[1] - int(ei[1].min()))
    pairs = int((sizes * (sizes - 1) // 2).sum())            # before the pairs shared by several hyperedges are merged
    res = dict(shape=shape, n=n, d=d, incidences=int(ei.shape[1]), max_size=int(sizes.max()), pairs_before_merging=pairs)
    run_explicit = pairs <= pair_limit
    if not run_explicit:
        res["explicit"] = f"not run: {pairs} pairs exceed --pair-limit {pair_limit}"

    def build_explicit():
        data = norm_contruction(ConstructV2V(SimpleNamespace(edge_index=ei)), TYPE='V2V')
        return data

    def build_implicit():
        return ImplicitCEGraph(ConstructV2V_implicit(SimpleNamespace(edge_index=ei)).edge_index, n)

    b_new, b_old, b_csr = [], [], []
    im = ex = None
    for _ in range(build_repeats):                            # alternate; the first round also warms both arms' allocations
        ms, im = _event_ms(build_implicit)
        b_new.append(ms)
        if run_explicit:
            ex = data = None                                  # (free the previous round's graph first)
            ms, data = _event_ms(build_explicit)
            b_old.append(ms)
            ms, ex = _event_ms(lambda: CEGraph(data.edge_index, data.norm, n))
            b_csr.append(ms)
    res["build_implicit"] = _stat(b_new)
    if run_explicit:
        res["build_explicit_ConstructV2V_gcn_norm"] = _stat(b_old)
        res["build_explicit_CEGraph_csr"] = _stat(b_csr)
        res["v2v_edges_with_loops"] = int(ex.edge_index.shape[1])
    res["implicit_index_bytes"] = sum(t.numel() * t.element_size() for t in (im.e_rowptr, im.e_col, im.v_rowptr, im.v_pos, im.long_seg,
                                                                               im.dinv, im.r_self))
    if run_explicit:
        res["explicit_index_bytes"] = sum(t.numel() * t.element_size() for t in (
            ex.inc.by_dst.rowptr, ex.inc.by_dst.col, ex.inc.by_src.rowptr, ex.inc.by_src.col, ex.w_dst, ex.w_src))

    x = torch.randn(n, d, device=DEV)
    g = torch.randn(n, d, device=DEV)
    b = torch.randn(d, device=DEV)
    long = dict(long_seg=im.long_seg if im.n_long else None, n_long=im.n_long)

    def new_fwd():
        t = ops.scan_rows(im.e_rowptr, im.e_col, x, im.dinv, reverse=False, **long)
        return ops.scan_collect(im.v_rowptr, im.v_pos, t, x, im.r_self, im.dinv, b, "relu", 0.5, 7)

    def new_bwd():
        t = ops.scan_rows(im.e_rowptr, im.e_col, g, im.dinv, reverse=True, **long)
        return ops.scan_collect(im.v_rowptr, im.v_pos, t, g, im.r_self, im.dinv)

    arms = [("implicit_fwd", new_fwd), ("implicit_bwd", new_bwd)]
    if run_explicit:
        arms += [("explicit_fwd_hconv_fwd_w", lambda: ops.hconv_propagate_w(ex.inc.by_dst, x, n, ex.w_dst, b, "relu", 0.5, 7)),
                 ("explicit_bwd_hconv_fwd_w", lambda: ops.hconv_propagate_w(ex.inc.by_src, g, n, ex.w_src))]
    for _, fn in arms:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in arms}
    for _ in range(repeats):                                  # alternate the arms inside one process
        for name, fn in arms:
            ms[name].append(_block(fn, iters))
    for name, _ in arms:
        res[name] = _stat(ms[name])
    if run_explicit:
        nnz = int(ex.edge_index.shape[1])
        algo = nnz * (4 * d + 8) + (n + 1) * 4 + n * 4 * d
        for which in ("fwd", "bwd"):
            k = res[f"explicit_{which}_hconv_fwd_w"]
            k["algo_bytes"], k["frac_8TBs"] = algo, algo / (k["median_ms"] * 1e-3) / PEAK
            res[f"{which}_implicit_median_below_explicit_min"] = res[f"implicit_{which}"]["median_ms"] < k["min_ms"]

    for which, fn in (("fwd", new_fwd), ("bwd", new_bwd)):    # the new launches on their own
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        try:
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            summ = timer.summary()
        finally:
            ops.set_kernel_timer(None)
        for kernel in ("scan_rows", "scan_collect"):
            k = summ[kernel]
            res[f"{kernel}_{which}"] = dict(avg_ms=k["avg_ms"], algo_bytes=k["algo_bytes"],
                                            frac_8TBs=k["algo_bytes"] / (k["avg_ms"] * 1e-3) / PEAK)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="fixed16,zipf4096")
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--build-repeats", type=int, default=3)
    ap.add_argument("--pair-limit", type=int, default=400_000_000)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "shapes": []}
    for shape in a.shapes.split(","):
        res["shapes"].append(measure(shape, a.n, a.d, a.repeats, a.iters, a.build_repeats, a.pair_limit))
        torch.cuda.empty_cache()
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
