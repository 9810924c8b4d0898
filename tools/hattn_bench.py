"""Timing of the hypergraph attention hop of HCHA's HypergraphConv(use_attention=True) (csrc/hattn.hip).

|V| = |E| = 1M, hyperedges of size 16 (uniform random members), H * F = 128 at H = 1 and 4: every launch of the forward (coefficient,
V->E hop, E->V hop with bias + elu + dropout 0.5) and of the backward (epilogue, E->V transposed, the vertex-major pass, the
hyperedge-major segment sum) on its own -- milliseconds (median of ``--reps`` repetitions of ``--iters`` calls, with the min..max
spread), algorithmic bytes and their fraction of 8 TB/s -- then forward + backward of ``functional.hattn_propagate`` through autograd,
and in the same run the same math as a torch composition on the same device (index_select, segment softmax by scatter, index_add_)
forward + backward.

    python tools/hattn_bench.py [--log2n 20] [--reps N] [--iters N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import Incidence, dense, hattn_propagate, ops  # noqa: E402

DEV = torch.device("cuda:0")
PEAK = 8.0e12


def _time(fn, reps=5, iters=5, warm=2):
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


def run(log2n, reps, iters):
    n, k, d = 1 << log2n, 16, 128
    g = torch.Generator(device=DEV).manual_seed(0)
    v = torch.randint(0, n, (n * k,), device=DEV, generator=g)
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    inc = Incidence.from_edge_index(torch.stack([v, e]), n_src=n, n_dst=n)
    nnz = inc.nnz
    pos = inc.pos_dst_of_src()
    deg = torch.bincount(v, minlength=n).float()
    D = torch.where(deg > 0, 1.0 / deg, torch.zeros_like(deg))
    B = torch.full((n,), 1.0 / k, device=DEV)
    out = {"n_v": n, "n_e": n, "nnz": nnz, "width": d}
    z = torch.randn(n, d, device=DEV)
    b = torch.randn(d, device=DEV)
    gy = torch.randn(n, d, device=DEV)
    for H in (1, 4):
        C = d // H
        av = torch.randn(n, H, device=DEV)
        ae = torch.randn(n, H, device=DEV)
        r = {}
        t = lambda fn: _time(fn, reps, iters)
        r["coef"] = _line(t(lambda: ops.hattn_coef(inc.by_src, pos, av, ae, 0.2, 0.5, 3)), nnz * (8 + 12 * H) + n * 12 * H)
        a_v, a_e, m, l = ops.hattn_coef(inc.by_src, pos, av, ae, 0.2, 0.5, 3)
        a_hop = nnz * (4 * d + 4 * H + 4) + n * 4 * d
        r["hop_v2e"] = _line(t(lambda: ops.hattn_hop(inc.by_dst, a_e, z, H, n, s=B)), a_hop)
        y_e = ops.hattn_hop(inc.by_dst, a_e, z, H, n, s=B)
        r["hop_e2v_epilogue"] = _line(t(lambda: ops.hattn_hop(inc.by_src, a_v, y_e, H, n, s=D, bias=b, act="elu", p=0.5, seed=7)), a_hop)
        y = ops.hattn_hop(inc.by_src, a_v, y_e, H, n, s=D, bias=b, act="elu", p=0.5, seed=7)
        r["bwd_epilogue"] = _line(t(lambda: ops.hconv_bwd_epi(gy, y, "elu", 0.5, 7, None, True)), 3 * n * d * 4)
        gg, _ = ops.hconv_bwd_epi(gy, y, "elu", 0.5, 7, None, True)
        r["bwd_e2v_transposed"] = _line(t(lambda: ops.hattn_hop(inc.by_dst, a_e, gg, H, n, r=D)), a_hop + 4 * nnz)
        gye = ops.hattn_hop(inc.by_dst, a_e, gg, H, n, r=D)
        r["bwd_vertex"] = _line(t(lambda: ops.hattn_bwd_vertex(inc.by_src, pos, a_v, av, ae, m, l, 0.2, z, gg, y_e, gye, D, B)),
                                nnz * (8 * d + 12 * H + 16) + n * (12 * d + 8 * H))
        _, _, ge_e = ops.hattn_bwd_vertex(inc.by_src, pos, a_v, av, ae, m, l, 0.2, z, gg, y_e, gye, D, B)
        r["bwd_edge"] = _line(t(lambda: ops.hattn_bwd_edge(inc.by_dst, ge_e, n)), nnz * 4 * H + n * 4 * H)
        del a_v, a_e, y_e, y, gg, gye, ge_e

        zr, avr, aer, br = (x.clone().requires_grad_(True) for x in (z, av, ae, b))

        def fused():
            for x in (zr, avr, aer, br):
                x.grad = None
            (hattn_propagate(zr, avr, aer, inc, H, D, B, 0.2, True, bias=br, act="elu", p_attn=0.5, p=0.5) * gy).sum().backward()
        r["fused_fwd_bwd"] = t(fused)

        def composition():
            for x in (zr, avr, aer, br):
                x.grad = None
            lg = torch.nn.functional.leaky_relu(avr.index_select(0, v) + aer.index_select(0, e), 0.2)
            mx = torch.full((n, H), -float("inf"), device=DEV).scatter_reduce(0, v.unsqueeze(-1).expand(-1, H), lg.detach(), reduce="amax")
            ex = torch.exp(lg - mx.index_select(0, v))
            den = torch.zeros(n, H, device=DEV).index_add_(0, v, ex)
            a = dense.hash_dropout(ex / (den.index_select(0, v) + 1e-16), 0.5, True).unsqueeze(-1)
            Y = torch.zeros(n, H, C, device=DEV).index_add_(0, e, zr.view(n, H, C).index_select(0, v) * a) * B.view(-1, 1, 1)
            U = torch.zeros(n, H, C, device=DEV).index_add_(0, v, Y.index_select(0, e) * a) * D.view(-1, 1, 1)
            o = dense.hash_dropout(torch.nn.functional.elu(U.view(n, d) + br), 0.5, True)
            (o * gy).sum().backward()
        try:
            r["torch_composition_fwd_bwd"] = _time(composition, max(reps // 2, 1), iters=2, warm=1)
            r["speedup"] = r["torch_composition_fwd_bwd"]["ms"] / r["fused_fwd_bwd"]["ms"]
        except torch.OutOfMemoryError:
            r["torch_composition_fwd_bwd"] = "not measured (out of memory: [nnz, H * F] message tensors)"
        out[f"H{H}"] = r
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20, help="|V| = |E| = 2^log2n")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0)}
    res.update(run(a.log2n, a.reps, a.iters))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
