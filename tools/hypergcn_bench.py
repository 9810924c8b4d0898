"""Timing of the HyperGCN baseline's on-device structure build and two-pass hop (csrc/hypergcn.hip).

|V| = |E| = 2^20, hyperedges of size 16, d = 16, 64 and 128.  Per width, alternating in the same run:
  * the yardstick: the existing degree-scaled V->E + E->V pair (``ops.hconv_propagate`` over both CSRs with ``r`` / ``s`` scales:
    csrc/hconv.hip, which this work leaves byte-identical);
  * the HyperGCN hop (``ops.hypergcn_v2e`` + ``ops.hypergcn_e2v``, bias + relu epilogue) with and without mediators;
  * the structure build (projection + select + degree) from a [n, d] matrix.
Milliseconds (median of ``--reps`` repetitions of 10 calls, with the min..max spread), algorithmic bytes, the time ratio against the
ratio of algorithmic bytes, and the yardstick's own max / min spread.  Then a 2-layer training step (forward + backward, eager, 64
input features, 8 classes) in both fast settings.

    python tools/hypergcn_bench.py [--skip-steps] [--reps N] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from allset_amd import Incidence, ops  # noqa: E402
from allset_amd.functional import hypergcn_structure  # noqa: E402

DEV = torch.device("cuda:0")


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


def _incidence(n, k):
    """n hyperedges of k distinct members each: member j of hyperedge e is (e * 7919 + j * 104729 + (e >> 5)) mod n."""
    e = torch.arange(n, device=DEV).repeat_interleave(k)
    j = torch.arange(k, device=DEV).repeat(n)
    v = (e * 7919 + j * 104729 + (e >> 5)) % n
    return Incidence.from_edge_index(torch.stack([v, e]), n_src=n, n_dst=n)


def hops(reps):
    n, k = 1 << 20, 16
    inc = _incidence(n, k)
    nnz = inc.nnz
    out = {"n_vertices": n, "n_hyperedges": n, "incidences": nnz}
    g = torch.Generator(device=DEV).manual_seed(0)
    r_v, s_e = torch.rand(n, device=DEV, generator=g) + 0.5, torch.rand(n, device=DEV, generator=g) + 0.5
    for d in (16, 64, 128):
        x = torch.randn(n, d, device=DEV, generator=g)
        bias = torch.randn(d, device=DEV, generator=g)
        rv = torch.rand(d, device=DEV, generator=g)
        st = {m: hypergcn_structure(x, rv, inc, m) for m in (True, False)}
        pair_bytes = 2 * (nnz * (4 * d + 8) + (n + 1) * 4 + n * 4 * d) + 4 * n
        hop_bytes = {True: (nnz * (4 * d + 8) + (n + 1) * 4 + 12 * n + 2 * n * 4 * d) + (nnz * (4 * d + 4) + (n + 1) * 4 + 8 * n + 2 * n * 4 * d),
                     False: (2 * n * (4 * d + 4) + 12 * n + n * 4 * d) + (nnz * 4 + 2 * n * (4 * d + 4) + (n + 1) * 4 + 8 * n + 2 * n * 4 * d)}
        build_bytes = n * d * 4 + nnz * 12 + n * 20 + nnz * 24 + n * 12

        def pair():
            h = ops.hconv_propagate(inc.by_dst, x, n, r=r_v, s=s_e)
            return ops.hconv_propagate(inc.by_src, h, n, r=s_e, s=r_v, bias=bias, act="relu")

        def hop(m):
            s = st[m]
            pq = ops.hypergcn_v2e(inc.by_dst, s.S, s.I, s.w, s.dinv, x, m)
            return ops.hypergcn_e2v(inc.by_src, s.colx, pq, s.dinv, s.selfc, x, bias, "relu")
        t = _time_alternating({"hconv_pair": pair, "hypergcn_hop_mediators": lambda: hop(True),
                               "hypergcn_hop_no_mediators": lambda: hop(False),
                               "structure_build_mediators": lambda: hypergcn_structure(x, rv, inc, True)}, reps)
        base = t["hconv_pair"]
        r = dict(t)
        r["hconv_pair"]["algo_bytes"] = pair_bytes
        r["hypergcn_hop_mediators"]["algo_bytes"] = hop_bytes[True]
        r["hypergcn_hop_no_mediators"]["algo_bytes"] = hop_bytes[False]
        r["structure_build_mediators"]["algo_bytes"] = build_bytes
        for m, key in ((True, "hypergcn_hop_mediators"), (False, "hypergcn_hop_no_mediators")):
            r[f"bytes_ratio_{key}_over_pair"] = hop_bytes[m] / pair_bytes
            r[f"time_ratio_{key}_over_pair"] = t[key]["ms"] / base["ms"]
        r["hconv_pair_spread_max_over_min"] = base["ms_max"] / base["ms_min"]
        out[f"d{d}"] = r
        del x, st
    return out, inc


def steps(reps, inc):
    from allset_amd import dense
    from allset_amd.baselines import HyperGCN
    n, f, c = inc.n_src, 64, 8
    out = {}
    g = torch.Generator(device=DEV).manual_seed(1)
    data = SimpleNamespace(x=torch.randn(n, f, device=DEV, generator=g))
    y = torch.randint(0, c, (n,), device=DEV, generator=g)
    for fast in (True, False):
        args = SimpleNamespace(HyperGCN_mediators=True, HyperGCN_fast=fast, dropout=0.5, dname="synthetic")
        torch.manual_seed(0)
        model = HyperGCN(n, inc, None, f, 2, c, args).to(DEV).train()

        def step():
            model.zero_grad(set_to_none=True)
            with dense.deferred_param_grads():
                torch.nn.functional.cross_entropy(model(data), y).backward()
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        ms = [_window(step, 5) for _ in range(reps)]
        out[f"train_step_2layer_{'fast' if fast else 'reapproximate'}"] = dict(ms=statistics.median(ms), ms_min=min(ms), ms_max=max(ms))
    return out


def _commit():
    try:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        return subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=root, capture_output=True, text=True).stdout.strip() or None
    except OSError:
        return None


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-steps", action="store_true")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--commit", default=None, help="commit hash to record (default: git rev-parse, where there is a repository)")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "commit": a.commit or _commit()}
    h, inc = hops(a.reps)
    res.update(h)
    if not a.skip_steps:
        res.update(steps(a.reps, inc))
    print(json.dumps(res, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
