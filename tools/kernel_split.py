"""Launches of one kernel in a rocprofv3 kernel trace (rocpd sqlite database), grouped by the kernel that ran before each on
the same stream -- tells apart call sites that launch the same kernel on different shapes (grn_bwd_kernel behind
cnx_m_finish_kernel = a ConvNeXt32 block, behind pro_bwd_kernel = a generic block).

    python tools/kernel_split.py results.db grn_bwd_kernel
"""
import collections
import sqlite3
import sys


def short(n):
    return n.replace("void sty::", "").replace("sty::", "").split("(")[0][:60]


def main(path, pat):
    c = sqlite3.connect(path)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    q = "stream_id" if "stream_id" in cols else "queue_id"
    last = {}
    agg = collections.defaultdict(list)
    for s, e, st, n in c.execute(f"select start, end, {q}, name from kernels order by start"):
        if pat in n:
            agg[last.get(st, "-")].append((e - s) / 1e3)
        last[st] = short(n)
    print(f"# launches of {pat} by the kernel before them on the same stream (us)")
    print(f"{'calls':>7} {'avg_us':>9} {'min_us':>9} {'max_us':>9}  previous kernel")
    for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
        print(f"{len(v):7d} {sum(v) / len(v):9.2f} {min(v):9.2f} {max(v):9.2f}  {k}")


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
