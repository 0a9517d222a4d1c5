#!/usr/bin/env python3
"""Per-kernel totals from a rocprofv3 --kernel-trace database (<name>_results.db): calls, total / mean microseconds and share of the
kernel time, longest first -- what --stats writes as a CSV when the output format is csv.
    python tools/rocpd_kernel_stats.py results.db [--match SUBSTRING ...]"""
import sqlite3
import sys


def main():
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, count(*), sum(end - start) from kernels group by name order by sum(end - start) desc").fetchall()
    total = sum(r[2] for r in rows)
    print("%8s %12s %10s %7s  %s" % ("calls", "total_us", "mean_us", "share", "kernel"))
    for name, n, ns in rows:
        print("%8d %12.1f %10.2f %6.2f%%  %s" % (n, ns / 1e3, ns / 1e3 / n, 100.0 * ns / total, name))
    print("%8s %12.1f %10s %7s  all kernels" % ("", total / 1e3, "", ""))


if __name__ == "__main__":
    main()
