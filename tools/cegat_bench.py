"""Timing of the clique-expansion baseline CEGAT's attention hop (csrc/gat.hip).

1. On the graph tools/ce_bench.py uses (the clique expansion of 1M hyperedges of size 16 over 1M vertices; GATConv's loops on every
   vertex), H * C = 128 at H = 1 and 4: the fused forward hop (bias + relu + dropout 0.5 in the launch; inference form and the form
   that also writes the positive-logit rows for a backward), the backward (epilogue, statistics + gar, source pass; each and all),
   and in the same run (a) allset_hconv_fwd_w on the same CSR, the project's weighted hop, and (b) an unfused torch restatement on
   the device (index_select, leaky_relu, scatter softmax, index_add_).  Milliseconds (median of ``--reps`` repetitions of 10 calls,
   with the min..max spread), algorithmic bytes and their fraction of 8 TB/s.
2. Graphed CEGAT training steps (ms per replay) on Cora- and Citeseer-shaped synthetic hypergraphs.

    python tools/cegat_bench.py [--skip-large] [--reps N] [--out FILE]
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

from allset_amd import Incidence, dense, ops  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def _time(fn, reps=5, iters=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(iters):
            fn()
        e.record()
        torch.cuda.synchronize()
        ms.append(s.elapsed_time(e) / iters)
    return dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))


def _line(t, algo):
    return dict(t, algo_bytes=int(algo), frac_8TBs=algo / (t["ms"] * 1e-3) / PEAK)


def large(reps):
    from allset_amd.baselines import CEGATGraph
    from allset_amd.preprocessing import ConstructV2V, norm_contruction
    n, k, d = 1 << 20, 16, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randint(0, n, (n * k,), device=DEV, generator=g)
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    data = norm_contruction(ConstructV2V(SimpleNamespace(edge_index=torch.stack([v, e]))), TYPE='V2V')
    graph = CEGATGraph(data.edge_index, n)
    del data, v, e
    inc = graph.inc
    nnz = inc.nnz
    out = {"attention_edges_with_loops": nnz, "n": n, "width": d}
    x = torch.randn(n, d, device=DEV)
    b = torch.randn(d, device=DEV)
    gy = torch.randn(n, d, device=DEV)
    w = torch.rand(nnz, device=DEV)
    out["hconv_fwd_w_same_csr"] = _line(_time(lambda: ops.hconv_propagate_w(inc.by_dst, x, n, w, b, "relu", 0.5, 7), reps),
                                        nnz * (4 * d + 8) + (n + 1) * 4 + n * 4 * d)
    del w
    for H in (1, 4):
        al = torch.randn(n, H, device=DEV)
        ar = torch.randn(n, H, device=DEV)
        r = {}
        a_inf = nnz * (4 * d + 4 * H + 4) + (n + 1) * 4 + n * (4 * d + 12 * H)
        r["fwd_inference"] = _line(_time(lambda: ops.gat_fwd(inc.by_dst, x, al, ar, H, 0.2, n, True, b, "relu", 0.5, 7), reps), a_inf)
        r["fwd_training"] = _line(_time(lambda: ops.gat_fwd(inc.by_dst, x, al, ar, H, 0.2, n, True, b, "relu", 0.5, 7, want_grad=True), reps),
                                  a_inf + n * (4 * d + 4 * H))
        y, _, aggpos, ppos, m, l = ops.gat_fwd(inc.by_dst, x, al, ar, H, 0.2, n, True, b, "relu", 0.5, 7, want_grad=True)
        r["bwd_epilogue"] = _line(_time(lambda: ops.hconv_bwd_epi(gy, y, "relu", 0.5, 7, None, True), reps), 3 * n * d * 4)
        gg, _ = ops.hconv_bwd_epi(gy, y, "relu", 0.5, 7, None, True)
        r["bwd_stats_and_gar"] = _line(_time(lambda: ops.gat_bwd_stats(gg, aggpos, ppos, m, l, 0.2, y=y, bias=b, p=0.5), reps),
                                       3 * n * d * 4 + n * H * 24)
        stats, _ = ops.gat_bwd_stats(gg, aggpos, ppos, m, l, 0.2, y=y, bias=b, p=0.5)
        a_src = nnz * (4 * d + 12 * H + 4) + (n + 1) * 4 + n * (8 * d + 8 * H)
        r["bwd_src"] = _line(_time(lambda: ops.gat_bwd_src(inc.by_src, x, al, ar, gg, stats, 0.2), reps), a_src)

        def bwd_all():
            g_, _ = ops.hconv_bwd_epi(gy, y, "relu", 0.5, 7, None, True)
            st, _ = ops.gat_bwd_stats(g_, aggpos, ppos, m, l, 0.2, y=y, bias=b, p=0.5)
            ops.gat_bwd_src(inc.by_src, x, al, ar, g_, st, 0.2)
        r["bwd_all_passes"] = _line(_time(bwd_all, reps), a_src + 6 * n * d * 4 + n * H * 24)
        del y, aggpos, gg, stats
        src, dst = graph.attention_index[0], graph.attention_index[1]
        C = d // H

        def unfused():
            e_ = torch.nn.functional.leaky_relu(al.index_select(0, src) + ar.index_select(0, dst), 0.2)
            mx = torch.full((n, H), -float("inf"), device=DEV).scatter_reduce(0, dst.unsqueeze(-1).expand(-1, H), e_, reduce="amax")
            ex = torch.exp(e_ - mx.index_select(0, dst))
            den = torch.zeros(n, H, device=DEV).index_add_(0, dst, ex)
            p_ = ex / (den.index_select(0, dst) + 1e-16)
            msg = x.view(n, H, C).index_select(0, src) * p_.unsqueeze(-1)
            y_ = torch.zeros(n, H, C, device=DEV).index_add_(0, dst, msg).view(n, d)
            return dense.hash_dropout(torch.relu(y_ + b), 0.5, True)
        try:
            r["fwd_unfused_torch"] = _time(unfused, max(reps // 2, 1), iters=2, warm=1)
        except torch.OutOfMemoryError:
            r["fwd_unfused_torch"] = "not measured (out of memory: [nnz, H * C] message tensor)"
        out[f"H{H}"] = r
    return out


def graphed_steps(reps):
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    from allset_amd.train import build_model, build_parser, preprocess, synthetic_dataset
    out = {}
    for method, extra in (("CEGCN", []), ("CEGAT", []), ("CEGAT", ["--heads", "4"])):
        for name, (n_v, n_e, f, c) in {"cora": (2708, 1579, 1433, 7), "citeseer": (3312, 1079, 3703, 6)}.items():
            args = build_parser().parse_args(["--method", method] + extra)
            data = preprocess(args, synthetic_dataset(n_v=n_v, n_e=n_e, num_classes=c, num_features=f, seed=0))
            args.num_features, args.num_classes = f, c
            model = build_model(args, data).to(DEV)
            data = data.to(DEV)
            y = data.y.long()
            step = GraphedTrainStep(model, data, lambda o: torch.nn.functional.cross_entropy(o, y), FusedAdam(model.parameters(), lr=0.001))
            out[f"{name}_{method}{'_heads4' if extra else ''}_graphed_step"] = _time(step, reps, iters=200, warm=10)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_large:
        res.update(large(a.reps))
    res.update(graphed_steps(a.reps))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
