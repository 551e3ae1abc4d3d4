#!/usr/bin/env python3
"""Kernel time of evaluate_kernel<P> per batch size from a rocprofv3 --kernel-trace database (the run of
`tools/evalbench.py --no-torch` under rocprofv3): dispatches, median / min µs, FLOP/s and share of the MFMA peak.

    python tools/nn_trace_summary.py TRACE.db
"""
import sqlite3
import statistics
import sys

FLOP_PER_BOARD = 373248
PEAK = {0: ("f32", 157.3e12, 64), 1: ("bf16", 2.5e15, 128)}     # precision -> (name, peak, boards per workgroup)


def main(path):
    c = sqlite3.connect(path)
    rows = c.execute("select name, grid_x, workgroup_x, duration, vgpr_count, accum_vgpr_count, lds_size, scratch_size "
                     "from kernels where name like '%evaluate_kernel%'").fetchall()
    groups = {}
    for name, gx, wx, dur, vg, ag, lds, scr in rows:
        prec = 1 if "ILi1E" in name or "<1>" in name else 0
        groups.setdefault((prec, gx // wx), []).append((dur, vg, ag, lds, scr))
    for (prec, wgs), d in sorted(groups.items()):
        pname, peak, m = PEAK[prec]
        us = [x[0] / 1e3 for x in d]
        med = statistics.median(us)
        boards = wgs * m
        print("%-4s workgroups %7d (<= %8d boards)  dispatches %3d  kernel us median %9.2f min %9.2f  %.3g FLOP/s = %.3f of "
              "peak  vgpr %d agpr %d lds %d scratch %d" % (pname, wgs, boards, len(d), med, min(us),
                                                           FLOP_PER_BOARD * boards / (med * 1e-6),
                                                           FLOP_PER_BOARD * boards / (med * 1e-6) / peak, *d[0][1:]))


if __name__ == "__main__":
    main(sys.argv[1])
