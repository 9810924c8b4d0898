#!/usr/bin/env python
"""The cell-row forward gather against the mask-row one at the headline shape: 1M x 1M, degree 16, d = 128,
the table relu + dropout 0.5 of random normals.  Times (HIP events, median / min / max of --iters launches after --warmup)

  * pack_rows writing mask rows against cell rows;
  * segreduce_packed over mask rows against cell rows, over both CSRs of the incidence -- V->E, where every row has
    `degree` incidences, and E->V, where the row lengths scatter around it;
  * the fused Linear that writes mask rows (csrc/fused_fwd2.hip mode 3) against the one that writes cell rows (mode 4);
  * with --variants DIR: the cell gather rebuilt with other step shapes (loads in flight / loads per LDS sub-step / waves per SIMD)
    and with 16-byte zero stores instead of clearing through the scatter addresses.  `--build-variants` compiles them into DIR
    (no GPU needed) and exits;

back to back ("hot") and with 1 GiB of unrelated memory written between launches ("cold").  Every result is first checked to be
bitwise the dense gather's.  Kill criterion, per direction, hot and cold: the cell gather must beat the mask gather by more than three
times the spread (max - min) of the mask gather's own repeats.

usage: python tools/cell_gather_bench.py [--variants DIR] [--out profiles/cell_gather_bench.txt]
Every GPU step is a child process under its own `timeout`; the first one that fails ends the run."""
import argparse
import ctypes
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
ap.add_argument("--variants", default=None, help="directory of the rebuilt cell gathers (see --build-variants)")
ap.add_argument("--build-variants", action="store_true", help="compile the variants into --variants and exit")
ap.add_argument("--out", default=None)
ap.add_argument("--step", default=None, choices=["hot", "cold"], help="(internal) run one GPU step and print its JSON line")
args = ap.parse_args()
D, P = 128, 0.5
# name -> (loads in flight, loads per sub-step, waves per SIMD, 16-byte zero stores)
VARIANTS = {"4 loads, 16 images, 4 waves": (4, 4, 4, False), "2 loads, 8 images, 8 waves": (2, 2, 8, False),
            "4 loads, 8 images, 8 waves, zero16": (4, 2, 8, True)}


def variant_path(name: str) -> str:
    q, h, w, z = VARIANTS[name]
    return os.path.join(args.variants, f"cellgather_q{q}h{h}w{w}{'z' if z else ''}.so")


def build_variants() -> int:
    os.makedirs(args.variants, exist_ok=True)
    src = [os.path.join(ROOT, "allset_amd", "csrc", f) for f in ("segreduce.hip", "abi.hip")]
    procs = []
    for name, (q, h, w, z) in VARIANTS.items():
        flags = [f"-DALLSET_CELL_LOADS={q}", f"-DALLSET_CELL_SUBSTEP={h}", f"-DALLSET_CELL_WAVES={w}"] + (["-DALLSET_CELL_ZERO16"] if z else [])
        procs.append(subprocess.Popen(["hipcc", "-O3", "-std=c++17", "--offload-arch=gfx950", "-fno-slp-vectorize", "-shared", "-fPIC",
                                       "-I", os.path.join(ROOT, "include"), "-o", variant_path(name)] + flags + src))
    return max(p.wait() for p in procs)


def gpu_step(cold: bool) -> dict:
    import torch
    from allset_amd import Incidence, dense, ops
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
    packed, cells = ops.pack_rows(x, fmt="mask"), ops.pack_rows(x, fmt="cells")
    dirs = (("V->E", inc.by_dst), ("E->V", inc.by_src))
    stream = torch.cuda.current_stream().cuda_stream
    P_, I64, I = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    variants = {}
    if args.variants:
        for name in VARIANTS:
            lib = ctypes.CDLL(variant_path(name))
            lib.allset_segreduce_cells_fwd.argtypes = [I, P_, P_, P_, P_, P_, I64, P_, I64, I64, I64, I64, P_]
            variants[name] = lib
    out_v = torch.empty(n, D, device=dev)

    def run_variant(lib, csr):
        rc = lib.allset_segreduce_cells_fwd(0, csr.row_order.data_ptr() if csr.row_order is not None else None, csr.rowptr.data_ptr(),
                                            csr.col.data_ptr(), cells.data_ptr(), x.data_ptr(), D, out_v.data_ptr(), D, n, n, D, stream)
        assert rc == 0
        return out_v

    equal = True
    for _, csr in dirs:
        want, _ = ops.segreduce(0, csr.rowptr, csr.col, None, x, n, variant=1, row_order=csr.row_order)
        for got in [ops.segreduce_packed(0, csr.rowptr, csr.col, packed, x, n, row_order=csr.row_order, fmt="mask"),
                    ops.segreduce_packed(0, csr.rowptr, csr.col, cells, x, n, row_order=csr.row_order, fmt="cells")] + \
                   [run_variant(lib, csr) for lib in variants.values()]:
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

    res = {"pack rows": timeit(lambda: ops.pack_rows(x, fmt="mask")), "pack cells": timeit(lambda: ops.pack_rows(x, fmt="cells"))}
    for name, csr in dirs:
        res["mask " + name] = timeit(lambda: ops.segreduce_packed(0, csr.rowptr, csr.col, packed, x, n, row_order=csr.row_order, fmt="mask"))
        res["cells " + name] = timeit(lambda: ops.segreduce_packed(0, csr.rowptr, csr.col, cells, x, n, row_order=csr.row_order, fmt="cells"))
        for vname, lib in variants.items():
            res[f"cells {name} [{vname}]"] = timeit(lambda: run_variant(lib, csr))

    # the two producers in the fused Linear's epilogue
    xl = torch.randn(n, D, device=dev, generator=g)
    W = torch.randn(D, D, device=dev, generator=g) / D ** 0.5
    bias = 0.1 * torch.randn(D, device=dev, generator=g)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    mask = torch.empty(dense.activation_mask_words(n, D), dtype=torch.int32, device=dev)
    arith = dense._arith_for(0, D, D, True, 0)
    lin = {"linear mask rows": lambda: ops.fused_linear_fwd_packed(xl, W, bias, gamma, beta, 1e-5, True, P, 101, True, P, 202, None, mask, arith, fmt="mask"),
           "linear cell rows": lambda: ops.fused_linear_fwd_packed(xl, W, bias, gamma, beta, 1e-5, True, P, 101, True, P, 202, None, mask, arith, fmt="cells")}
    y = dense.fused_linear_fwd(xl, W, bias, gamma, beta, 1e-5, True, P, 101, True, P, 202, None, mask)[0]
    lc, side, _ = lin["linear cell rows"]()
    over = (y.view(torch.int32) != 0).sum(1) > 48
    rows_equal = bool(torch.equal(lc, ops.pack_rows(y, fmt="cells"))) and bool(torch.equal(side.view(torch.int32)[over], y.view(torch.int32)[over]))
    del y, lc, side
    for name, fn in lin.items():
        res[name] = timeit(fn)
    deg = inc.by_src.rowptr[1:] - inc.by_src.rowptr[:-1]
    return {"step": "cold" if cold else "hot", "n": n, "nnz": nnz, "bitwise_equal": equal, "linear_rows_equal": rows_equal,
            "occupied_mean": float(occupied.float().mean()), "occupied_max": int(occupied.max()),
            "over48": int((occupied > 48).sum()), "over60": int((occupied > 60).sum()), "linear_over48": int(over.sum()),
            "ev_max_degree": int(deg.max()), "kernels": res}


def table(rows) -> str:
    out = []
    for r in rows:
        k = r["kernels"]
        nnz, n = r["nnz"], r["n"]
        req = nnz * 2 + n * 4 + nnz * 4 // 128                       # 128-byte lines: rows gathered + rows written + column ids
        out.append(f"[{r['step']}] n = {n}, nnz = {nnz}, d = {D}; occupied columns per row: mean {r['occupied_mean']:.1f}, max "
                   f"{r['occupied_max']}; rows above 48 (cell overflow): {r['over48']} = {r['over48'] / n:.2e} of the table, above 60 (mask "
                   f"overflow): {r['over60']}; every gather bitwise equal to the dense one: {r['bitwise_equal']}")
        out.append(f"  the Linear's output: rows above 48: {r['linear_over48']}; mode-4 rows equal to the packed cell rows of the dense output, side table "
                   f"holds the overflow rows: {r['linear_rows_equal']}")
        out.append(f"  E->V row lengths: max {r['ev_max_degree']} (V->E: all {nnz // n})")
        out.append(f"  {'kernel':<58}{'median ms':>10}{'min':>9}{'max':>9}{'G lines/s':>11}")
        for name, t in k.items():
            lines = req if (name.startswith("mask ") or name.startswith("cells ")) else n * 6 if name.startswith("pack") else 0
            rate = f"{lines / t['median'] / 1e6:>11.1f}" if lines else ""
            out.append(f"  {name:<58}{t['median']:>10.3f}{t['min']:>9.3f}{t['max']:>9.3f}{rate}")
        for d in ("V->E", "E->V"):
            mask, cell = k["mask " + d], k["cells " + d]
            spread = mask["max"] - mask["min"]
            gain = mask["median"] - cell["median"]
            out.append(f"  {d}: cell gather {cell['median']:.3f} ms against mask gather {mask['median']:.3f} ms: gain {gain:+.3f} ms, mask spread "
                       f"(max - min of {args.iters}) {spread:.3f} ms, criterion gain > 3 x spread: {'PASS' if gain > 3 * spread else 'FAIL'}")
        out.append(f"  packing cell rows against mask rows: {k['pack cells']['median'] - k['pack rows']['median']:+.3f} ms; the Linear writing cell rows "
                   f"against mask rows: {k['linear cell rows']['median'] - k['linear mask rows']['median']:+.3f} ms per launch")
    return "\n".join(out) + "\n"


def main() -> int:
    if args.build_variants:
        return build_variants()
    if args.step is not None:
        print("RESULT " + json.dumps(gpu_step(args.step == "cold")), flush=True)
        return 0
    rows = []
    for step in ("hot", "cold"):
        cmd = ["timeout", "-k", "10", str(args.step_timeout), sys.executable, os.path.abspath(__file__), "--step", step, "--n", str(args.n),
               "--degree", str(args.degree), "--iters", str(args.iters), "--warmup", str(args.warmup)]
        if args.variants:
            cmd += ["--variants", args.variants]
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
