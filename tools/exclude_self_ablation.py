"""Exclude-self aggregation: leave-one-out sums over the unexpanded incidence (csrc/loo.hip) against the expansion path
(``preprocessing.expand_edge_index`` + the ordinary ``deepsets_aggregate``), one V->E + E->V pair, forward + backward, d = 128.

    python tools/exclude_self_ablation.py [--out profiles/exclude_self_ablation.json] [--repeats 5] [--iters 20]

Method (hipEvent medians): per shape both paths are warmed up, then ``--repeats`` times alternately each path runs ``--iters`` timed
pairs, every pair between two events on the launch stream; the figure of a repeat is the median over its pairs, the reported time
the median over the repeats, the spread their (max - min).  The ``loo_rows`` launches are timed on their own through
``ops.KernelTimer`` (events around the entry point) and set against the 8 TB/s roofline with the algorithmic bytes
``nnz * (2 * d * 4 + 4) + (n_seg + 1) * 4`` per pass (the second read of a long segment's rows is expected to hit cache).  Shapes:
|V| = |E| = 250k with size-16 hyperedges, and the Zipf <= 4096 generator of ``allset_amd.synthetic`` at the largest size whose
expansion fits (the expansion is skipped, and said to be, where it does not).  ``--counters``: one pass of each ``loo_rows`` form only,
for a counters-only ``rocprofv3 --pmc`` run of this script.  ``--attention [--heads 4]``: the same protocol and shapes for the PMA pooling
-- ``pma_aggregate_exclude_self`` (the leave-one-out softmax of csrc/loo_softmax.hip) against ``pma_aggregate``
over the expansion, with the ``loo_softmax_fwd`` / ``loo_softmax_bwd`` launches timed on their own."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import (Incidence, LeaveOneOutIncidence, deepsets_aggregate, deepsets_aggregate_exclude_self, ops,  # noqa: E402
                        pma_aggregate, pma_aggregate_exclude_self)
from allset_amd import preprocessing as P                                                                          # noqa: E402
from allset_amd.synthetic import random_hypergraph                                                                 # noqa: E402

HBM_BYTES_PER_S = 8.0e12
EXPANSION_LIMIT = 400_000_000          # expanded incidences: 16 B of int64 ids each before the CSRs are built, and int32 positions


def _pair_times(fn, iters: int):
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def measure(name: str, n_v: int, n_e: int, dist: str, degree: float, d: int, repeats: int, iters: int, dev, heads: int = 0) -> dict:
    """``heads`` > 0: the PMA pooling with that many heads instead of the Deep Sets sum."""
    hg = random_hypergraph(n_v, n_e, degree=degree, seed=0, device=dev, dist=dist, e_base=n_v)
    ei = hg.edge_index
    sizes = torch.bincount(ei[1] - n_v)
    n_exp = int((sizes * (sizes - 1)).sum() + (sizes == 1).sum())
    loo = LeaveOneOutIncidence(ei, n_v=n_v, e_base=n_v)
    x = torch.randn(n_v, d, device=dev, requires_grad=True)
    G = torch.randn(loo.n_dst, d, device=dev)

    if heads:
        a_v = torch.randn(n_v, heads, device=dev, requires_grad=True)
        a_e = torch.randn(loo.nnz, heads, device=dev, requires_grad=True)
        loo.merge_incidence()

    def new_pair():
        if heads:
            y = pma_aggregate_exclude_self(x, a_v, loo, "v2e", heads)
            out = pma_aggregate_exclude_self(y, a_e, loo, "e2v", heads)
            torch.autograd.grad(out, (x, a_v, a_e), G)
            return
        y = deepsets_aggregate_exclude_self(x, loo, "v2e", "add")
        out = deepsets_aggregate_exclude_self(y, loo, "e2v", "add")
        torch.autograd.grad(out, x, G)

    res = dict(shape=name, n_v=n_v, n_e=n_e, nnz=int(loo.nnz), max_size=int(loo.max_size), d=d, expanded_incidences=n_exp)
    old_pair = None
    if n_exp <= EXPANSION_LIMIT:
        data = P.expand_edge_index(SimpleNamespace(edge_index=ei.clone(), n_x=[n_v], num_hyperedges=[n_e]))
        eie = data.edge_index
        eie[1] -= n_v
        inc = Incidence.from_edge_index(eie, n_src=n_v)
        rev = inc.reversed()
        del data, eie

        def old_pair():
            if heads:
                y, _, _ = pma_aggregate(x, a_v, inc, heads)
                out, _, _ = pma_aggregate(y, a_e, rev, heads)
                torch.autograd.grad(out, (x, a_v, a_e), G)
                return
            y = deepsets_aggregate(x, inc, None, "add")
            out = deepsets_aggregate(y, rev, None, "add")
            torch.autograd.grad(out, x, G)
    else:
        res["expansion"] = f"not run: {n_exp} expanded incidences exceed the {EXPANSION_LIMIT} this tool builds"

    for fn in (new_pair, old_pair):
        if fn is not None:
            for _ in range(3):
                fn()
    torch.cuda.synchronize()
    new_ms, old_ms = [], []
    for _ in range(repeats):                                   # alternate the two versions inside one process
        new_ms.append(_pair_times(new_pair, iters))
        if old_pair is not None:
            old_ms.append(_pair_times(old_pair, iters))
    res.update(new_ms=statistics.median(new_ms), new_ms_spread=max(new_ms) - min(new_ms), new_ms_repeats=new_ms)
    if old_ms:
        res.update(expansion_ms=statistics.median(old_ms), expansion_ms_spread=max(old_ms) - min(old_ms), expansion_ms_repeats=old_ms,
                   ratio=statistics.median(old_ms) / statistics.median(new_ms))

    timer = ops.KernelTimer()
    ops.set_kernel_timer(timer)
    try:
        for _ in range(iters):
            new_pair()
        torch.cuda.synchronize()
        summ = timer.summary()
    finally:
        ops.set_kernel_timer(None)
    if heads:
        res["heads"] = heads
        for kernel, per_row in (("loo_softmax_fwd", 2 * d + 2 * heads), ("loo_softmax_bwd", 4 * d + 4 * heads)):
            k = summ[kernel]
            algo = loo.nnz * (per_row * 4 + 2) + (loo.n_e + 1) * 4          # (col: 4 bytes in the V->E launch, none in the E->V one)
            res.update({f"{kernel}_avg_ms": k["avg_ms"], f"{kernel}_calls_per_pair": k["calls"] / iters, f"{kernel}_algo_bytes": algo,
                        f"{kernel}_roofline_fraction": algo / HBM_BYTES_PER_S / (k["avg_ms"] * 1e-3)})
        return res
    k = summ["loo_rows"]
    algo = loo.nnz * (2 * d * 4 + 4) + (loo.n_e + 1) * 4
    res.update(loo_rows_avg_ms=k["avg_ms"], loo_rows_calls_per_pair=k["calls"] / iters, loo_rows_algo_bytes=algo,
               loo_rows_roofline_fraction=algo / HBM_BYTES_PER_S / (k["avg_ms"] * 1e-3),
               segreduce_avg_ms=summ["segreduce_fwd"]["avg_ms"],
               segreduce_roofline_fraction=summ["segreduce_fwd"]["algo_bytes"] / HBM_BYTES_PER_S / (summ["segreduce_fwd"]["avg_ms"] * 1e-3))
    return res


def counters_pass(d: int, dev) -> None:
    n = 250_000
    hg = random_hypergraph(n, n, degree=16, seed=0, device=dev, dist="fixed", e_base=n)
    loo = LeaveOneOutIncidence(hg.edge_index, n_v=n, e_base=n)
    x = torch.randn(n, d, device=dev)
    for _ in range(2):
        y = ops.loo_rows(loo.e_rowptr, loo.e_col, x, n_long=0)
        ops.loo_rows(loo.e_rowptr, None, y, n_long=0)
    torch.cuda.synchronize()
    print(json.dumps(dict(counters_pass=True, nnz=int(loo.nnz), d=d, algo_bytes_per_pass=loo.nnz * (2 * d * 4 + 4) + (loo.n_e + 1) * 4)))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--counters", action="store_true")
    ap.add_argument("--attention", action="store_true", help="time the PMA pooling (leave-one-out softmax) instead of the Deep Sets sum")
    ap.add_argument("--heads", type=int, default=4)
    args = ap.parse_args()
    heads = args.heads if args.attention else 0
    if not torch.cuda.is_available():
        raise SystemExit("exclude_self_ablation: needs the GPU (nothing here is measured on a CPU)")
    dev = torch.device("cuda:0")
    if args.counters:
        counters_pass(args.d, dev)
        return
    results = [measure("fixed16_250k", 250_000, 250_000, "fixed", 16, args.d, args.repeats, args.iters, dev, heads)]
    torch.cuda.empty_cache()
    # Zipf sizes up to 4096 (mean 16): one 4096-member hyperedge alone expands to 16.7M incidences
    for n in (250_000, 60_000, 15_000):
        r = measure(f"zipf4096_{n // 1000}k", n, n, "zipf", 16, args.d, args.repeats, args.iters, dev, heads)
        results.append(r)
        torch.cuda.empty_cache()
        if "expansion_ms" in r:
            break
    for r in results:
        print(json.dumps(r))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(tool="tools/exclude_self_ablation.py", repeats=args.repeats, iters=args.iters, results=results), f, indent=1)


if __name__ == "__main__":
    main()
