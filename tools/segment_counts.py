#!/usr/bin/env python
"""Static instruction counts per barrier-to-barrier segment of one kernel, from the compiler's assembly (no GPU needed).

    python tools/segment_counts.py allset_amd/csrc/fused_bwd6.hip --list
    python tools/segment_counts.py allset_amd/csrc/fused_bwd6.hip fused_linear_bwd_f16x3_kernelILb1ELb0ELb0ELb0ELb0ELb0ELb0E

The file is compiled for the device only with build.CXXFLAGS -S.  A kernel is named by a substring of its mangled symbol; its text is
cut at every s_barrier and at every loop header (marked L: what stands before it is the loop's set-up, not a tick), in program order,
and each piece gets one row: lines by mnemonic prefix (v_mfma, other v_, s_, ds_, global_) and the opcodes that mark address
bookkeeping (s_nop, v_mov_b32, v_mad_u64_u32, v_mul_lo_u32, 64-bit v_cmp).  The order of the roles in the text is the compiler's (in
fused_bwd6.hip the matrix waves' loop comes first); the loops are where the segments repeat.  Counts are static: a segment that spans
a branch counts both sides, and the scheduler may move instructions across a barrier that only orders memory.  The kernel's register
and scratch figures follow the table."""
import argparse, os, re, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from allset_amd import build  # noqa: E402

NAMED = ("s_nop", "v_mov_b32", "v_mad_u64_u32", "v_mul_lo_u32")
CMP64 = re.compile(r"^v_cmpx?_\w+_[iuf]64")


def assembly(path, extra):
    cmd = [build._hipcc()] + build.CXXFLAGS + list(extra) + ["--cuda-device-only", "-S", "-o", "-", path]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if res.returncode != 0:
        raise SystemExit(res.stderr)
    return res.stdout.splitlines()


def kernels(lines):
    """{symbol: (first line, last line)} of every function in the text"""
    out, cur, start = {}, None, 0
    for i, ln in enumerate(lines):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):", ln)
        if m and not ln.startswith(".L") and cur is None and i > 0 and ".type" in " ".join(lines[max(0, i - 6):i]):
            cur, start = m.group(1), i
        elif cur is not None and ln.startswith(".Lfunc_end"):
            out[cur] = (start, i)
            cur = None
    return out


def count(seg):
    c = {"v_mfma": 0, "v_": 0, "s_": 0, "ds_": 0, "global_": 0, "cmp64": 0}
    c.update({k: 0 for k in NAMED})
    for ln in seg:
        t = ln.strip()
        if not t or t[0] in ".;" or t.endswith(":"):
            continue
        op = t.split()[0]
        if op.startswith("v_mfma"):
            c["v_mfma"] += 1
        elif op.startswith("v_"):
            c["v_"] += 1
        elif op.startswith("s_"):
            c["s_"] += 1
        elif op.startswith("ds_"):
            c["ds_"] += 1
        elif op.startswith("global_"):
            c["global_"] += 1
        for k in NAMED:
            if op == k or op.startswith(k + "_"):
                c[k] += 1
        if CMP64.match(op):
            c["cmp64"] += 1
    return c


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("source")
    ap.add_argument("symbol", nargs="?", help="substring of the kernel's mangled name")
    ap.add_argument("--list", action="store_true", help="print the kernel symbols of the file and stop")
    ap.add_argument("-D", action="append", default=[], help="extra -D flags")
    a = ap.parse_args()
    lines = assembly(a.source, ["-D" + d for d in a.D])
    ks = kernels(lines)
    if a.list or not a.symbol:
        print("\n".join(ks))
        return
    hits = [k for k in ks if a.symbol in k]
    if len(hits) != 1:
        raise SystemExit(f"{len(hits)} symbols match {a.symbol!r}: {hits}")
    lo, hi = ks[hits[0]]
    body = lines[lo:hi]
    cuts = [i for i, ln in enumerate(body) if ln.strip().split()[:1] == ["s_barrier"] or "Loop Header: Depth=1" in ln and ln.startswith(".LBB")]
    print(f"# {hits[0]}")
    cols = ["v_mfma", "v_", "s_", "ds_", "global_"] + list(NAMED) + ["cmp64"]
    print("seg  " + " ".join(f"{c:>13s}" for c in cols))
    prev = 0
    for s, cut in enumerate(cuts + [len(body)]):
        c = count(body[prev:cut])
        print(f"{s:3d}{'L' if prev and body[prev - 1].startswith('.LBB') else ' '} " + " ".join(f"{c[k]:13d}" for k in cols))
        prev = cut + 1
    for ln in lines[hi:hi + 60]:
        if re.search(r"; (NumVgprs|NumAgprs|TotalNumVgprs|NumSgprs|ScratchSize|Occupancy|codeLenInByte)", ln):
            print("#" + ln.strip()[1:])


if __name__ == "__main__":
    main()
