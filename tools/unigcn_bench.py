"""Timing of the UniGCNII baseline's fused E->V hop (csrc/unigcn.hip).

1. |V| = |E| = 1M, hyperedges of size 16, d = 128 and 256: the fused hop (``ops.unigcn_hop_fwd``, with and without the row norm)
   and, alternating with it in the same run, the existing degree-scaled launch it extends (``ops.hconv_propagate`` over the same
   vertex-major CSR with ``s = degV``: csrc/hconv.hip, which this work leaves byte-identical) -- milliseconds (median of ``--reps``
   repetitions of 10 calls, with the min..max spread), algorithmic bytes and their fraction of 8 TB/s, the time ratio against the ratio of
   algorithmic bytes, and the unfused composition (hconv launch + torch ops for the norm and the residual).
2. A graphed UniGCNII training step (ms per replay) on a Cora-shaped synthetic hypergraph, ``--UniGNN_use-norm`` off and on.

    python tools/unigcn_bench.py [--skip-large] [--skip-steps] [--reps N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import Incidence, ops  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def _window(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def _time_alternating(fns, reps=7, iters=10, warm=3):
    """Median / min / max ms per call of every function, their windows interleaved (A B C A B C ...) so that what else runs on the
    machine meets all of them alike."""
    for fn in fns.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ms[k].append(_window(fn, iters))
    return {k: dict(ms=statistics.median(v), ms_min=min(v), ms_max=max(v)) for k, v in ms.items()}


def large(reps):
    n, k = 1 << 20, 16
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randint(0, n, (n * k,), device=DEV, generator=g)
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    inc = Incidence.from_edge_index(torch.stack([v, e]), n_src=n, n_dst=n)
    del v, e
    csr, nnz = inc.by_src, inc.nnz
    degV = torch.rand(n, device=DEV) + 0.5
    out = {"n_vertices": n, "n_hyperedges": n, "incidences": nnz}
    for d in (128, 256):
        xe, x0 = torch.randn(n, d, device=DEV), torch.randn(n, d, device=DEV)
        hconv_bytes = nnz * (4 * d + 4) + (n + 1) * 4 + n * 4 * d
        fused_bytes = hconv_bytes + n * 4 * d

        def unfused():
            a = ops.hconv_propagate(csr, xe, n, s=degV)
            nrm = a.norm(dim=1)
            t = torch.where(nrm > 0, 1.0 / nrm, torch.zeros_like(nrm))
            return torch.add(x0 * 0.1, a * t.unsqueeze(1), alpha=0.9)
        t = _time_alternating({"hconv_fwd_e2v": lambda: ops.hconv_propagate(csr, xe, n, s=degV),
                               "unigcn_hop": lambda: ops.unigcn_hop_fwd(csr, xe, x0, n, degV, 0.1, False),
                               "unigcn_hop_use_norm": lambda: ops.unigcn_hop_fwd(csr, xe, x0, n, degV, 0.1, True),
                               "unfused_hconv_plus_torch_use_norm": unfused}, reps)
        r = {kk: dict(vv, algo_bytes=int(hconv_bytes if kk == "hconv_fwd_e2v" else fused_bytes),
                      frac_8TBs=(hconv_bytes if kk == "hconv_fwd_e2v" else fused_bytes) / (vv["ms"] * 1e-3) / PEAK) for kk, vv in t.items()}
        base = t["hconv_fwd_e2v"]
        r["bytes_ratio_fused_over_hconv"] = fused_bytes / hconv_bytes
        r["time_ratio_hop_over_hconv"] = t["unigcn_hop"]["ms"] / base["ms"]
        r["time_ratio_hop_use_norm_over_hconv"] = t["unigcn_hop_use_norm"]["ms"] / base["ms"]
        r["hconv_spread_max_over_min"] = base["ms_max"] / base["ms_min"]
        out[f"d{d}"] = r
        del xe, x0
    return out


def graphed_steps(reps):
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.train import build_model, build_parser, make_optimizer, preprocess, synthetic_dataset
    out = {}
    for extra in ([], ["--UniGNN_use-norm"]):
        n_v, n_e, f, c = 2708, 1579, 1433, 7
        args = build_parser().parse_args(["--method", "UniGCNII"] + extra)
        data = preprocess(args, synthetic_dataset(n_v=n_v, n_e=n_e, num_classes=c, num_features=f, seed=0))
        args.num_features, args.num_classes = f, c
        model = build_model(args, data).to(DEV)
        data = data.to(DEV)
        args.UniGNN_degV, args.UniGNN_degE = args.UniGNN_degV.to(DEV), args.UniGNN_degE.to(DEV)
        y = data.y.long()
        step = GraphedTrainStep(model, data, lambda o: torch.nn.functional.cross_entropy(o, y), make_optimizer(args, model))
        for _ in range(10):
            step()
        torch.cuda.synchronize()
        ms = [_window(step, 200) for _ in range(reps)]
        out[f"cora_UniGCNII{'_use_norm' if extra else ''}_graphed_step"] = dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    if not a.skip_large:
        res.update(large(a.reps))
    if not a.skip_steps:
        res.update(graphed_steps(a.reps))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
