"""Timing of the clique-expansion baseline CEGCN (csrc/clique.hip, allset_hconv_fwd_w in csrc/hconv.hip).

1. The device clique expansion (ConstructV2V + norm_contruction(TYPE='V2V')) of the configs[2]-derived hypergraph: 1M vertices,
   1M hyperedges of size 16 (about 120M pairs before deduplication).
2. The GCN hop forward (weighted propagate + bias + relu + dropout 0.5) and its transposed gather (the backward) over that graph
   at C = 128: ms and the fraction of 8 TB/s of the algorithmic bytes nnz * (4C + 8) + (n + 1) * 4 + n * 4C, against the unfused
   torch restatement (index_select * w, index_add_, bias, relu, dropout).
3. Graphed CEGCN training steps (ms per replay) on Cora- and Citeseer-shaped synthetic hypergraphs.

    python tools/ce_bench.py [--skip-large] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import Incidence, dense, ops  # noqa: E402

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
    from allset_amd.preprocessing import ConstructV2V, norm_contruction
    n, k, d = 1 << 20, 16, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randint(0, n, (n * k,), device=DEV, generator=g)
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    out = {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    data = norm_contruction(ConstructV2V(SimpleNamespace(edge_index=torch.stack([v, e]))), TYPE='V2V')
    torch.cuda.synchronize()
    out["clique_expansion_and_gcn_norm_ms"] = (time.perf_counter() - t0) * 1e3      # (host clock around synchronised work)
    ei, w = data.edge_index, data.norm
    nnz = ei.shape[1]
    out["v2v_edges_with_loops"] = nnz
    inc = Incidence.from_edge_index(ei, n_src=n, n_dst=n)
    w_dst = w[inc.perm_dst_long()].contiguous()
    w_src = w[inc.perm_src_long()].contiguous()
    x = torch.randn(n, d, device=DEV)
    b = torch.randn(d, device=DEV)
    algo = nnz * (4 * d + 8) + (n + 1) * 4 + n * 4 * d
    ms = _time(lambda: ops.hconv_propagate_w(inc.by_dst, x, n, w_dst, b, "relu", 0.5, 7))
    out["gcn_hop_fwd"] = dict(ms=ms, frac_8TBs=algo / (ms * 1e-3) / PEAK)
    ms = _time(lambda: ops.hconv_propagate_w(inc.by_src, x, n, w_src))
    out["gcn_hop_transposed_gather"] = dict(ms=ms, frac_8TBs=algo / (ms * 1e-3) / PEAK)
    src, dst = ei[0], ei[1]

    def unfused():
        y = torch.zeros(n, d, device=DEV).index_add_(0, dst, x.index_select(0, src) * w.unsqueeze(-1))
        return dense.hash_dropout(torch.relu(y + b), 0.5, True)
    try:
        out["gcn_hop_unfused_torch_ms"] = _time(unfused, iters=5, warm=1)
    except torch.OutOfMemoryError:
        out["gcn_hop_unfused_torch_ms"] = "not measured (out of memory: [nnz, C] message tensor)"
    return out


def graphed_steps():
    from allset_amd.graphs import GraphedTrainStep
    from allset_amd.optim import FusedAdam
    from allset_amd.train import build_model, build_parser, preprocess, synthetic_dataset
    out = {}
    for name, (n_v, n_e, f, c) in {"cora": (2708, 1579, 1433, 7), "citeseer": (3312, 1079, 3703, 6)}.items():
        args = build_parser().parse_args(["--method", "CEGCN"])
        data = preprocess(args, synthetic_dataset(n_v=n_v, n_e=n_e, num_classes=c, num_features=f, seed=0))
        args.num_features, args.num_classes = f, c
        model = build_model(args, data).to(DEV)
        data = data.to(DEV)
        y = data.y.long()
        step = GraphedTrainStep(model, data, lambda o: torch.nn.functional.cross_entropy(o, y), FusedAdam(model.parameters(), lr=0.001))
        out[f"{name}_CEGCN_graphed_step_ms"] = _time(step, iters=200, warm=10)
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
