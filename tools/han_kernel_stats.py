"""Per-kernel times of ``tools/han_bench.py --trace-steps`` from a ``rocprofv3 --kernel-trace --stats`` run of its own (the rocpd SQLite
database that run writes), as CSV: the cross-check of the tool's HIP-event times.  The first ``--skip`` steps'
launches of every kernel are warm-up (code loading, allocator growth) and are left out: a kernel launched k times per step loses
its first ``k * skip`` launches.

    rocprofv3 --kernel-trace --stats -d OUT -o han -- python tools/han_bench.py --trace-steps 50 --warmup 10 --shape synthetic_1M
    python tools/han_kernel_stats.py OUT/han_results.db --skip 10 --steps 60 > profiles/han_kernel_stats_synthetic_1M.csv
"""
from __future__ import annotations

import argparse
import re
import sqlite3
import statistics


def short(name: str) -> str:
    return re.sub(r"\(.*", "", name).replace("void ", "").replace("allset::", "")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--skip", type=int, default=10, help="warm-up steps at the head of the trace")
    ap.add_argument("--steps", type=int, default=60, help="steps in the trace, warm-up included")
    a = ap.parse_args()
    rows = sqlite3.connect(a.db).execute("select name, duration from kernels order by start").fetchall()
    by = {}
    for n, d in rows:
        if "han::" in n:
            by.setdefault(short(n), []).append(d / 1000.0)
    print("kernel,launches_per_step,launches,avg_us,min_us,max_us,stddev_us,us_per_step")
    for k, us in sorted(by.items()):
        per = len(us) / a.steps
        kept = us[int(round(per * a.skip)):]
        print(f"\"{k}\",{per:g},{len(kept)},{statistics.mean(kept):.1f},{min(kept):.1f},{max(kept):.1f},{statistics.pstdev(kept):.1f},"
              f"{statistics.mean(kept) * per:.1f}")


if __name__ == "__main__":
    main()
