#!/usr/bin/env python
"""The packed-nonzero-row gather against the dense gather at the headline shape: 1M x 1M, degree 16, d = 128,
the table relu + dropout 0.5 of random normals.  Times the dense gather, the pack kernel and the packed gather (HIP events, median of
--iters launches after --warmup) over both CSRs of the incidence -- V->E, where every row has `degree` incidences, and E->V, where the
row lengths scatter around it --, back to back ("hot") and with 1 GiB of unrelated memory written between launches ("cold": the
Infinity Cache holds nothing of the previous repeat), and states the kill criterion per direction: pack + packed gather must beat the
dense gather by more than three times the spread (max - min) of the dense gather's own repeats.

usage: python tools/packed_gather_bench.py [--out profiles/packed_gather_bench.txt]
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
ap.add_argument("--step-timeout", type=int, default=240, help="seconds per GPU step")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["hot", "cold"], help="(internal) run one GPU step and print its JSON line")
args = ap.parse_args()
D = 128


def gpu_step(cold: bool) -> dict:
    import torch
    from allset_amd import Incidence, ops
    from allset_amd.synthetic import random_hypergraph
    dev = torch.device("cuda:0")
    n = args.n
    hg = random_hypergraph(n, n, args.degree, seed=11, device=dev, dist="fixed")
    inc = Incidence.from_edge_index(hg.edge_index, n_src=n, n_dst=n)
    nnz = int(inc.by_dst.col.numel())
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.relu(torch.randn(n, D, device=dev, generator=g))
    x = x * (torch.rand(n, D, device=dev, generator=g) >= 0.5).float() * 2.0
    occupied = (x != 0).sum(1)
    packed = ops.pack_rows(x, fmt="mask")
    # V->E: every row has exactly `degree` incidences; E->V (the transposed CSR): the rows' lengths scatter around it
    dirs = (("V->E", inc.by_dst), ("E->V", inc.by_src))
    equal = True
    for _, csr in dirs:
        want, _ = ops.segreduce(0, csr.rowptr, csr.col, None, x, n, variant=1, row_order=csr.row_order)
        got = ops.segreduce_packed(0, csr.rowptr, csr.col, packed, x, n, row_order=csr.row_order, fmt="mask")
        equal = equal and bool(torch.equal(got.view(torch.int32), want.view(torch.int32)))
        del want, got
    scrub = torch.empty(1 << 28, dtype=torch.float32, device=dev) if cold else None      # 1 GiB

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

    res = {"pack": timeit(lambda: ops.pack_rows(x, fmt="mask"))}
    for name, csr in dirs:
        res["dense " + name] = timeit(lambda: ops.segreduce(0, csr.rowptr, csr.col, None, x, n, variant=1, row_order=csr.row_order))
        res["packed " + name] = timeit(lambda: ops.segreduce_packed(0, csr.rowptr, csr.col, packed, x, n, row_order=csr.row_order, fmt="mask"))
    deg = inc.by_src.rowptr[1:] - inc.by_src.rowptr[:-1]
    return {"step": "cold" if cold else "hot", "n": n, "nnz": nnz, "bitwise_equal": equal,
            "occupied_mean": float(occupied.float().mean()), "occupied_max": int(occupied.max()),
            "overflow_rows": int((occupied > 60).sum()), "ev_max_degree": int(deg.max()), "kernels": res}


def table(rows) -> str:
    out = []
    for r in rows:
        k = r["kernels"]
        nnz, n = r["nnz"], r["n"]
        req_dense = nnz * 4 + n * 4 + nnz * 4 // 128                 # 128-byte lines: rows gathered + rows written + column ids
        req_packed = nnz * 2 + n * 4 + nnz * 4 // 128
        out.append(f"[{r['step']}] n = {n}, nnz = {nnz}, d = {D}; occupied columns per row: mean {r['occupied_mean']:.1f}, max "
                   f"{r['occupied_max']}, rows above 60: {r['overflow_rows']}; packed result bitwise equal to dense: {r['bitwise_equal']}")
        out.append(f"  E->V row lengths: max {r['ev_max_degree']} (V->E: all {nnz // n})")
        out.append(f"  {'kernel':<20}{'median ms':>10}{'min':>9}{'max':>9}{'G lines/s':>11}")

        def line(name, t, req):
            out.append(f"  {name:<20}{t['median']:>10.3f}{t['min']:>9.3f}{t['max']:>9.3f}{req / t['median'] / 1e6:>11.1f}")
        line("pack rows", k["pack"], n * 6)
        for d in ("V->E", "E->V"):
            line("dense gather " + d, k["dense " + d], req_dense)
            line("packed gather " + d, k["packed " + d], req_packed)
        for d in ("V->E", "E->V"):
            dense, both = k["dense " + d], k["pack"]["median"] + k["packed " + d]["median"]
            spread = dense["max"] - dense["min"]
            gain = dense["median"] - both
            out.append(f"  {d}: pack + packed gather {both:.3f} ms against dense {dense['median']:.3f} ms: gain {gain:+.3f} ms, dense spread "
                       f"(max - min of {args.iters}) {spread:.3f} ms, criterion gain > 3 x spread: {'PASS' if gain > 3 * spread else 'FAIL'}")
    return "\n".join(out) + "\n"


def main() -> int:
    if args.step is not None:
        print("RESULT " + json.dumps(gpu_step(args.step == "cold")), flush=True)
        return 0
    rows = []
    for step in ("hot", "cold"):
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
