"""One HAN training step (forward, cross-entropy, backward, Adam) with the HIP kernels of csrc/han.hip against the same model composed
from torch ops on the same GPU in the same process (index gathers, scatter_reduce / index_add_, torch.stack, nn.Sequential), at a
Cora-shaped hypergraph and a synthetic one with about 10^6 metapath edges per graph.  The yardstick is the torch-op composition; it
is timed twice (before and after the HIP path) and its run-to-run spread is reported beside the comparison.  Per entry point: the
time from HIP events (ops.KernelTimer) and the achieved fraction of its algorithmic bytes over 8 TB/s.

A timed window is at least ``--window`` seconds long (the step count is sized from a pilot after the warm-up).

    python tools/han_bench.py [--out profiles/han_bench.json]
    rocprofv3 --kernel-trace --stats -d OUT -o han -- python tools/han_bench.py --trace-steps 50 --shape synthetic_1M
    python tools/han_kernel_stats.py OUT/han_results.db --skip 10       (per-kernel times of a run of its own, warm-up steps dropped)
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from allset_amd import han, ops  # noqa: E402
from allset_amd.synthetic import random_hypergraph  # noqa: E402

DEV = torch.device("cuda:0")
HBM_BYTES_PER_S = 8e12


class TorchGATConv(nn.Module):
    def __init__(self, in_feats, out_feats, heads, p):
        super().__init__()
        self.H, self.C, self.p = heads, out_feats, p
        self.fc = nn.Linear(in_feats, out_feats * heads, bias=False)
        self.attn_l = nn.Parameter(torch.randn(1, heads, out_feats) * 0.3)
        self.attn_r = nn.Parameter(torch.randn(1, heads, out_feats) * 0.3)
        self.bias = nn.Parameter(torch.zeros(heads * out_feats))

    def forward(self, g, feat):
        n, H, C = feat.shape[0], self.H, self.C
        fs = self.fc(F.dropout(feat, self.p, self.training)).view(n, H, C)
        el, er = (fs * self.attn_l).sum(-1), (fs * self.attn_r).sum(-1)
        e = F.leaky_relu(el[g.src] + er[g.dst], 0.2)
        idx = g.dst.view(-1, 1).expand(-1, H)
        mx = torch.full((n, H), -float("inf"), device=e.device).scatter_reduce(0, idx, e.detach(), "amax")
        ex = torch.exp(e - mx[g.dst])
        a = ex / torch.zeros((n, H), device=e.device).index_add_(0, g.dst, ex)[g.dst]
        a = F.dropout(a, self.p, self.training)
        rst = torch.zeros((n, H, C), device=e.device).index_add_(0, g.dst, fs[g.src] * a.unsqueeze(-1))
        return F.elu(rst + self.bias.view(1, H, C))


class TorchHAN(nn.Module):
    def __init__(self, M, in_size, hidden, out_size, heads, p):
        super().__init__()
        self.convs = nn.ModuleList([TorchGATConv(in_size, hidden, heads, p) for _ in range(M)])
        self.project = nn.Sequential(nn.Linear(hidden * heads, 128), nn.Tanh(), nn.Linear(128, 1, bias=False))
        self.predict = nn.Linear(hidden * heads, out_size)

    def forward(self, gs, h):
        z = torch.stack([conv(g, h).flatten(1) for conv, g in zip(self.convs, gs)], dim=1)
        beta = torch.softmax(self.project(z).mean(0), dim=0)
        return self.predict((beta.expand((z.shape[0],) + beta.shape) * z).sum(1))


def shapes():
    rng = np.random.default_rng(0)
    n_v, n_e = 2708, 1579
    vs, es = [], []
    for e in range(n_e):
        k = int(rng.integers(2, 9))
        vs += rng.choice(n_v, size=k, replace=False).tolist()
        es += [e] * k
    cora = dict(name="cora_shaped", n_v=n_v, n_e=n_e, F=1433, C=7, edge_index=torch.tensor([vs, es], device=DEV))
    hg = random_hypergraph(16000, 16000, degree=8, seed=1, device=DEV)
    syn = dict(name="synthetic_1M", n_v=16000, n_e=16000, F=64, C=5, edge_index=hg.edge_index)
    return [cora, syn]


def make_step(model, gs, x, y, mask):
    opt = torch.optim.Adam(model.parameters(), lr=0.005, weight_decay=0.001)
    loss_fn = nn.CrossEntropyLoss()

    def step():
        model.train()
        loss = loss_fn(model(gs, x)[mask], y[mask])
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return step


def time_step(step, warmup, window_s, repeats):
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        step()
    e.record()
    torch.cuda.synchronize()
    steps = max(20, int(np.ceil(window_s * 1e3 / (s.elapsed_time(e) / 10))))
    out = []
    for _ in range(repeats):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(steps):
            step()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) / steps)
    return out, steps


def setup(shape):
    from types import SimpleNamespace
    n_v, n_e = shape["n_v"], shape["n_e"]
    gs = han.metapath_graphs(SimpleNamespace(edge_index=shape["edge_index"], n_x=[n_v], num_hyperedges=[n_e]))
    g = torch.Generator(device=DEV).manual_seed(0)
    x = torch.cat([torch.randn(n_v, shape["F"], device=DEV, generator=g), torch.zeros(n_e, shape["F"], device=DEV)])
    y = torch.randint(0, shape["C"], (n_v + n_e,), device=DEV, generator=g)
    mask = torch.zeros(n_v + n_e, dtype=torch.bool, device=DEV)
    mask[:n_v // 2] = True
    torch.manual_seed(0)
    hip = han.HAN(2, shape["F"], 8, shape["C"], [8], 0.6).to(DEV)
    ref = TorchHAN(2, shape["F"], 8, shape["C"], 8, 0.6).to(DEV)
    return gs, make_step(hip, gs, x, y, mask), make_step(ref, gs, x, y, mask)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--window", type=float, default=0.6, help="least length of a timed window, seconds")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--shape", default=None, help="only this shape")
    ap.add_argument("--trace-steps", type=int, default=0, help="only run this many steps of the HIP path, after --warmup more (for "
                    "rocprofv3; tools/han_kernel_stats.py drops the warm-up launches)")
    a = ap.parse_args()
    results = []
    for shape in shapes():
        if a.shape and shape["name"] != a.shape:
            continue
        gs, hip_step, ref_step = setup(shape)
        if a.trace_steps:
            for _ in range(a.warmup + a.trace_steps):
                hip_step()
            torch.cuda.synchronize()
            continue
        ref_a, ref_steps = time_step(ref_step, a.warmup, a.window, a.repeats)
        hip, hip_steps = time_step(hip_step, a.warmup, a.window, a.repeats)
        ref_b, _ = time_step(ref_step, a.warmup, a.window, a.repeats)
        timer = ops.KernelTimer()
        ops.set_kernel_timer(timer)
        for _ in range(50):
            hip_step()
        torch.cuda.synchronize()
        ops.set_kernel_timer(None)
        kernels = {k: dict(v, frac_of_8TBps=v["algo_bytes"] / (v["avg_ms"] * 1e-3) / HBM_BYTES_PER_S)
                   for k, v in timer.summary().items() if k.startswith("han_")}
        ref_all = ref_a + ref_b
        r = dict(shape=shape["name"], steps_per_window=dict(hip=hip_steps, torch=ref_steps), nodes=shape["n_v"] + shape["n_e"], edges=[g.nnz for g in gs], hip_ms=hip, torch_ms_before=ref_a,
                 torch_ms_after=ref_b, hip_median_ms=float(np.median(hip)), torch_median_ms=float(np.median(ref_all)),
                 torch_spread_ms=float(max(ref_all) - min(ref_all)), kernels=kernels)
        r["not_slower"] = r["hip_median_ms"] <= r["torch_median_ms"] + r["torch_spread_ms"]
        results.append(r)
        print(json.dumps(r), flush=True)
    if a.out and results:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
