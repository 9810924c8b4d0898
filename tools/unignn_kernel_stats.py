"""Per-arm kernel times of ``tools/unignn_bench.py --skip-steps`` from a ``rocprofv3 --kernel-trace --stats`` run of its own (the
rocpd SQLite database that run writes), as CSV: the cross-check of the tool's HIP-event times.

The bench interleaves its arms, so one kernel name pools several arms (the three K1 arms are all ``unignn_rows_kernel<.., VertexTail>``).
The trace is therefore cut by position: kernels in start order, grouped into runs of one name; a run of 10 launches (11 for the
pooling arms, 30 for the three K1 arms, split 10 / 10 / 10 in the tool's order) is one timed window, shorter runs are warm-up and are
left out.  Arms whose launches alternate with torch kernels (the unfused compositions) form no runs and are not listed.

    rocprofv3 --kernel-trace --stats -d OUT -o unignn -- python tools/unignn_bench.py --skip-steps --reps 3
    python tools/unignn_kernel_stats.py OUT/unignn_results.db > profiles/unignn_kernel_stats.csv
"""
from __future__ import annotations

import itertools
import re
import sqlite3
import statistics
import sys

K1_ARMS = ("k1_gcn_norm_relu_drop", "k1_gin_self_norm_relu_drop", "k1_sage_self_plain")


def short(name: str) -> str:
    return re.sub(r"\(.*", "", name).replace("void ", "").replace("allset::", "")


def main(path: str) -> None:
    rows = sqlite3.connect(path).execute("select name, duration from kernels order by start").fetchall()
    runs = [(k, [d / 1000.0 for _, d in g]) for k, g in itertools.groupby(((short(n), d) for n, d in rows), key=lambda t: t[0])]
    arms = {}                                                 # (lanes per row, arm, kernel) -> [us]
    reps_of_k1 = max(sum(1 for k, us in runs if "VertexTail" in k and len(us) == 30 and f"<{w}," in k) for w in (32, 64))
    seen_k1 = {}
    for k, us in runs:
        m = re.search(r"<(?:float, )?(?:4, )?(\d+)", k)
        lpr = int(m.group(1)) if m else 0
        if "VertexTail" in k and len(us) == 30:
            seen_k1[lpr] = seen_k1.get(lpr, 0) + 1
            for i, arm in enumerate(K1_ARMS):
                arms.setdefault((lpr, arm, k), []).extend(us[10 * i:10 * i + 10])
        elif "EdgeLogit" in k and len(us) == 10:
            arms.setdefault((lpr, "k2_v2e_att", k), []).extend(us)
        elif "hconv_fwd_kernel" in k and len(us) == 10:
            # the bare launch opens every repetition of its group: e2v (before the K1 arms) first, v2e (before K2) once K1 is done
            arm = "hconv_fwd_v2e" if seen_k1.get(lpr, 0) >= reps_of_k1 else "hconv_fwd_e2v"
            arms.setdefault((lpr, arm, k), []).extend(us)
        elif "pma_fwd_kernel" in k and len(us) == 11:
            arms.setdefault((lpr, "pma_fwd_e2v_and_tail_arms_pooled", k), []).extend(us)
    print("d,arm,kernel,launches,avg_us,min_us,max_us,stddev_us")
    for (lpr, arm, k), us in arms.items():
        print(f"{lpr * 4},{arm},\"{k}\",{len(us)},{statistics.mean(us):.1f},{min(us):.1f},{max(us):.1f},{statistics.pstdev(us):.1f}")


if __name__ == "__main__":
    main(sys.argv[1])
