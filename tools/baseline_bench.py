"""Timing of the hypergraph-convolution baselines (csrc/hconv.hip).

1. ``hconv_fwd`` (V->E with r, s, bias, ELU, dropout) and the transposed gather of the backward on the configs[2]-shaped hypergraph
   (1M vertices, 1M hyperedges of size 16, d = 128): ms and the fraction of 8 TB/s of the algorithmic bytes
   (nnz * (4d + 4) + (n_t + 1) * 4 + n_t * 4d, + 4 nnz for r).
2. The same fused hop against the weighted ``segreduce`` (per-incidence weight r[col]) + torch scale / bias / ELU / dropout.
3. Graphed HCHA and HNHN training steps (ms per replay) on Cora- and Citeseer-shaped synthetic hypergraphs.

    python tools/baseline_bench.py [--skip-large]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import Incidence, dense, ops  # noqa: E402
from allset_amd._lib import SUM  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def _time(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def large():
    n, k, d = 1 << 20, 16, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randint(0, n, (n * k,), device=DEV, generator=g)
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    inc = Incidence.from_edge_index(torch.stack([v, e]), n_src=n, n_dst=n)
    x = torch.randn(n, d, device=DEV)
    r = torch.rand(n, device=DEV)
    s = torch.rand(n, device=DEV)
    b = torch.randn(d, device=DEV)
    nnz = n * k
    out = {}
    algo = nnz * (4 * d + 4 + 4) + (n + 1) * 4 + n * 4 * d
    ms = _time(lambda: ops.hconv_propagate(inc.by_dst, x, n, r, s, b, "elu", 0.5, 7))
    out["hconv_fwd_v2e"] = dict(ms=ms, frac_8TBs=algo / (ms * 1e-3) / PEAK)
    ms = _time(lambda: ops.hconv_propagate(inc.by_src, x, n, r=s, s=r))
    out["hconv_transposed_gather"] = dict(ms=ms, frac_8TBs=algo / (ms * 1e-3) / PEAK)
    algo_seg = nnz * (4 * d + 8) + (n + 1) * 4 + n * 4 * d
    w = r[inc.by_dst.col.long()].contiguous()                        # r as a per-incidence weight (CSR order)
    ms = _time(lambda: ops.segreduce(SUM, inc.by_dst.rowptr, inc.by_dst.col, None, x, n, variant=1))
    out["segreduce_sum_same_shape"] = dict(ms=ms, frac_8TBs=(algo_seg - 4 * nnz) / (ms * 1e-3) / PEAK)

    def unfused():
        y, _ = ops.segreduce(SUM, inc.by_dst.rowptr, inc.by_dst.col, w, x, n, variant=1)
        y = torch.nn.functional.elu(s.unsqueeze(-1) * y + b)
        return dense.hash_dropout(y, 0.5, True)
    out["unfused_segreduce_torch_epilogue_ms"] = _time(unfused)
    out["fused_hconv_ms"] = out["hconv_fwd_v2e"]["ms"]
    return out


def graphed_steps():
    from allset_amd.baselines import HCHA, HNHN
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    from allset_amd.train import build_parser, preprocess, synthetic_dataset
    out = {}
    for name, (n_v, n_e, f, c) in {"cora": (2708, 1579, 1433, 7), "citeseer": (3312, 1079, 3703, 6)}.items():
        for method in ("HCHA", "HNHN"):
            args = build_parser().parse_args(["--method", method])
            data = synthetic_dataset(n_v=n_v, n_e=n_e, num_classes=c, num_features=f, seed=0)
            data = preprocess(args, data)
            args.num_features, args.num_classes = f, c
            model = (HCHA if method == "HCHA" else HNHN)(args).to(DEV)
            data = data.to(DEV)
            y = data.y.long()
            opt = FusedAdam(model.parameters(), lr=0.001)
            step = GraphedTrainStep(model, data, lambda o: torch.nn.functional.cross_entropy(o, y), opt)
            out[f"{name}_{method}_graphed_step_ms"] = _time(step, iters=200, warm=10)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_large:
        res.update(large())
    res.update(graphed_steps())
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
