"""Build time and peak device memory of the metapath graphs: the boolean sparse product (csrc/metapath.hip through
``han_hetero.metapath_reachable_edges``) against the torch expansion it stands beside (``han.metapath_edges``, the yardstick), in one
process.  One call of ``han.metapath_edges`` builds BOTH two-step graphs of an incidence (X Y X and Y X Y), so each shape is measured as
that pair on both paths, from the int64 edge lists to int64 edge lists: PAP + APA and PFP + FPF of the synthetic typed graph
(``synthetic.acm_like_hetero`` at the size printed in the result), VEV + EVE of tools/han_bench.py's synthetic hypergraph.  The new
path's time includes building the relations' CSR.  Per shape and path: the median and min - max over ``--windows`` builds (after one
warm-up build) and the peak of ``torch.cuda.max_memory_allocated`` above what was allocated before the build.  "not slower" only if the
new path's median is below the yardstick's FASTEST window.

    python tools/metapath_bench.py [--out profiles/metapath_bench.json]"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allset_amd import han  # noqa: E402
from allset_amd.han_hetero import HeteroGraph, metapath_reachable_edges  # noqa: E402
from allset_amd.synthetic import acm_like_hetero, random_hypergraph  # noqa: E402

DEV = torch.device("cuda:0")
TYPED = dict(n_papers=20000, n_authors=25000, n_fields=60, seed=0)


def measure(build, windows):
    out, peak = [], 0
    for i in range(windows + 1):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t0 = time.perf_counter()
        res = build()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        peak = max(peak, torch.cuda.max_memory_allocated() - base)
        edges = [int(r[0].numel()) for r in res]
        del res
        if i > 0:
            out.append(dt)
    return dict(median_ms=float(np.median(out)), min_ms=float(min(out)), max_ms=float(max(out)), windows=len(out),
                peak_bytes=int(peak), edges=edges)


def shape(name, x, y, n_x, n_y, windows):
    """The incidence ``x[i] -- y[i]`` between ``n_x`` and ``n_y`` nodes: X Y X and Y X Y on both paths."""
    def hip():
        g = HeteroGraph({("x", "xy", "y"): (x, y), ("y", "yx", "x"): (y, x)}, {"x": n_x, "y": n_y})
        return [metapath_reachable_edges(g, ["xy", "yx"])[:2], metapath_reachable_edges(g, ["yx", "xy"])[:2]]

    def torch_path():
        return han.metapath_edges(torch.stack([x, y]), n_x, n_y)

    deg = torch.bincount(y, minlength=n_y).double()
    degx = torch.bincount(x, minlength=n_x).double()
    r = dict(name=name, n_x=n_x, n_y=n_y, incidences=int(x.numel()), candidates=int((deg * deg).sum() + (degx * degx).sum()),
             torch=measure(torch_path, windows), hip=measure(hip, windows))
    r["torch"]["edges"] = [e - (n_x + n_y) for e in r["torch"]["edges"]]            # (its appended self-loops)
    assert r["torch"]["edges"] == r["hip"]["edges"], r
    r["not_slower"] = r["hip"]["median_ms"] < r["torch"]["min_ms"]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metapath_bench.json"))
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    d = acm_like_hetero(device=DEV, **TYPED)
    pa, pf = d.edges[("paper", "pa", "author")], d.edges[("paper", "pf", "field")]
    hg = random_hypergraph(16000, 16000, degree=8, seed=1, device=DEV)
    results = [shape("typed PAP + APA", pa[0], pa[1], TYPED["n_papers"], TYPED["n_authors"], a.windows),
               shape("typed PFP + FPF", pf[0], pf[1], TYPED["n_papers"], TYPED["n_fields"], a.windows),
               shape("hypergraph VEV + EVE (han_bench synthetic_1M)", hg.edge_index[0], hg.edge_index[1], 16000, 16000, a.windows)]
    out = dict(device=torch.cuda.get_device_name(0), typed_graph=TYPED, results=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    for r in results:
        print(f"{r['name']}: hip {r['hip']['median_ms']:.1f} ms ({r['hip']['min_ms']:.1f} - {r['hip']['max_ms']:.1f}), peak "
              f"{r['hip']['peak_bytes'] / 2 ** 20:.1f} MiB | torch {r['torch']['median_ms']:.1f} ms ({r['torch']['min_ms']:.1f} - "
              f"{r['torch']['max_ms']:.1f}), peak {r['torch']['peak_bytes'] / 2 ** 20:.1f} MiB | {r['candidates']} candidates, "
              f"{sum(r['hip']['edges'])} edges | not slower: {r['not_slower']}")


if __name__ == "__main__":
    main()
