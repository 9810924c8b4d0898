#!/usr/bin/env python
"""The fused Linear that writes packed rows from its epilogue (csrc/fused_fwd2.hip mode 3) against the pair it replaces, at the
headline shape: [n, 128] behind a LayerNorm, dropout 0.5 in and out, fp32, auto arithmetic.

  (a) the dense <LayerNorm, dropout in, relu + dropout out> Linear followed by ops.pack_rows of its output;
  (b) the packed-mode Linear;
  (c) a check that the packed gather over (b)'s buffer is bitwise the dense gather over (a)'s table.

Same protocol as tools/packed_gather_bench.py: HIP events, median / min / max of --iters launches after --warmup, back to back ("hot")
and with 1 GiB of unrelated memory written between launches ("cold").  Kill criterion: (a) - (b) must exceed three times the spread
(max - min) of (a)'s own repeats, hot and cold.  --sweep: the same at powers of two from 1024 rows (hot only), for the row count from
which functional.set_packed_epilogue("auto") takes the fused route.

usage: python tools/packed_epilogue_bench.py [--sweep] [--out profiles/packed_epilogue_bench.txt]
Every GPU step is a child process under its own `timeout`; the first one that fails ends the run."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=1_000_000)
ap.add_argument("--degree", type=int, default=16)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--sweep", action="store_true", help="also time powers of two from 1024 to 65536 rows (hot)")
ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["hot", "cold", "sweep"], help="(internal) run one GPU step and print its JSON line")
args = ap.parse_args()
D, P = 128, 0.5
SWEEP = (1024, 2048, 4096, 8192, 16384, 32768, 65536)


def _time_pair(n: int, scrub, check_gather: bool) -> dict:
    import torch
    from allset_amd import Incidence, dense, ops
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn(n, D, device=dev, generator=g)
    W = torch.randn(D, D, device=dev, generator=g) / D ** 0.5
    bias = 0.1 * torch.randn(D, device=dev, generator=g)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    mask = torch.empty(dense.activation_mask_words(n, D), dtype=torch.int32, device=dev)
    arith = dense._arith_for(0, D, D, True, 0)

    def lin_dense():
        return dense.fused_linear_fwd(x, W, bias, gamma, beta, 1e-5, True, P, 101, True, P, 202, None, mask)[0]

    def lin_packed():
        return ops.fused_linear_fwd_packed(x, W, bias, gamma, beta, 1e-5, True, P, 101, True, P, 202, None, mask, arith, fmt="mask")

    def timeit(fn):
        ts = []
        for i in range(args.warmup + args.iters):
            if scrub is not None:
                scrub.fill_(float(i))
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); torch.cuda.synchronize()
            if i >= args.warmup:
                ts.append(s.elapsed_time(e))
        return {"median": statistics.median(ts), "min": min(ts), "max": max(ts)}

    y = lin_dense()
    packed_ref = ops.pack_rows(y, fmt="mask")
    packed, side, _ = lin_packed()
    occupied = (y.view(torch.int32) != 0).sum(1)
    fits = occupied <= 60
    same_rows = bool(torch.equal(packed[:, :4], packed_ref[:, :4])) and bool(torch.equal(packed[fits], packed_ref[fits])) and \
        bool(torch.equal(side.view(torch.int32)[~fits], y.view(torch.int32)[~fits]))
    res = {"n": n, "occupied_mean": float(occupied.float().mean()), "occupied_max": int(occupied.max()),
           "overflow_rows": int((~fits).sum()), "rows_equal": same_rows}
    if check_gather:
        from allset_amd.synthetic import random_hypergraph
        hg = random_hypergraph(n, n, args.degree, seed=11, device=dev, dist="fixed")
        inc = Incidence.from_edge_index(hg.edge_index, n_src=n, n_dst=n)
        equal = True
        for csr in (inc.by_dst, inc.by_src):
            want, _ = ops.segreduce(0, csr.rowptr, csr.col, None, y, n, variant=1, row_order=csr.row_order)
            got = ops.segreduce_packed(0, csr.rowptr, csr.col, packed, side, n, row_order=csr.row_order, fmt="mask")
            equal = equal and bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
            del want, got
        res["gather_equal"] = equal
        del hg, inc
    res["kernels"] = {"linear dense": timeit(lin_dense), "pack rows": timeit(lambda: ops.pack_rows(y, fmt="mask")),
                      "linear + pack": timeit(lambda: ops.pack_rows(lin_dense(), fmt="mask")), "linear packed": timeit(lin_packed)}
    return res


def gpu_step(step: str):
    import torch
    if step == "sweep":
        return {"step": step, "sizes": [_time_pair(n, None, False) for n in SWEEP]}
    scrub = torch.empty(1 << 28, dtype=torch.float32, device="cuda:0") if step == "cold" else None      # 1 GiB
    return {"step": step, **_time_pair(args.n, scrub, True)}


def _verdict(k) -> str:
    a, b = k["linear + pack"], k["linear packed"]
    gain, spread = a["median"] - b["median"], a["max"] - a["min"]
    return (f"(a) {a['median']:.3f} ms - (b) {b['median']:.3f} ms: gain {gain:+.3f} ms, spread of (a) (max - min of {args.iters}) "
            f"{spread:.3f} ms, criterion gain > 3 x spread: {'PASS' if gain > 3 * spread else 'FAIL'}")


def table(rows) -> str:
    out = []
    for r in rows:
        if r["step"] == "sweep":
            out.append("[sweep, hot] rows: (a) Linear + pack_rows, (b) packed-mode Linear, median ms (min .. max)")
            for s in r["sizes"]:
                k = s["kernels"]
                a, b = k["linear + pack"], k["linear packed"]
                out.append(f"  n = {s['n']:>6}: (a) {a['median']:.4f} ({a['min']:.4f} .. {a['max']:.4f})  (b) {b['median']:.4f} "
                           f"({b['min']:.4f} .. {b['max']:.4f})  rows equal: {s['rows_equal']}  " + _verdict(k))
            continue
        k = r["kernels"]
        out.append(f"[{r['step']}] n = {r['n']}, d = {D}, dropout {P} in and out; occupied columns per row: mean {r['occupied_mean']:.1f}, max "
                   f"{r['occupied_max']}, rows above 60: {r['overflow_rows']}; packed rows equal to pack_rows of the dense output: "
                   f"{r['rows_equal']}; (c) packed gather over (b) bitwise the dense gather over (a), both CSRs: {r['gather_equal']}")
        out.append(f"  {'kernel':<34}{'median ms':>10}{'min':>9}{'max':>9}")
        for name in ("linear dense", "pack rows", "linear + pack", "linear packed"):
            t = k[name]
            label = {"linear + pack": "(a) dense Linear, then pack_rows", "linear packed": "(b) packed-mode Linear",
                     "linear dense": "dense Linear alone", "pack rows": "pack_rows alone"}[name]
            out.append(f"  {label:<34}{t['median']:>10.3f}{t['min']:>9.3f}{t['max']:>9.3f}")
        out.append("  " + _verdict(k))
        out.append(f"  packed-mode Linear against its dense twin alone: {k['linear packed']['median'] - k['linear dense']['median']:+.3f} ms")
    return "\n".join(out) + "\n"


def main() -> int:
    if args.step is not None:
        print("RESULT " + json.dumps(gpu_step(args.step)), flush=True)
        return 0
    rows = []
    for step in ("hot", "cold") + (("sweep",) if args.sweep else ()):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n),
               "--degree", str(args.degree), "--iters", str(args.iters), "--warmup", str(args.warmup)]
        res = subprocess.run(cmd, capture_output=True, text=True)
        line = [l for l in res.stdout.splitlines() if l.startswith("RESULT ")]
        if res.returncode != 0 or not line:
            sys.stderr.write(res.stdout[-4000:] + res.stderr[-4000:])
            print(f"step {step} ended with status {res.returncode}: nothing further is started on the GPU", flush=True)
            return res.returncode or 1
        rows.append(json.loads(line[-1][len("RESULT "):]))
    text = table(rows)
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
