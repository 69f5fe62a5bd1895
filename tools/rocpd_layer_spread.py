#!/usr/bin/env python3
"""Per-position min / median / max of the kernels of a U-Net evaluation from a rocprofv3 rocpd database
(the passes rocpd_layers.py reports by their median): the spread a before / after comparison of one layer
has to exceed.  usage: rocpd_layer_spread.py run_results.db [out.txt]"""
import collections
import sqlite3
import statistics
import sys

from rocpd_layers import short


def main() -> int:
    db = sqlite3.connect(sys.argv[1])
    rows = db.execute("select name, start, end, grid_x from kernels order by start").fetchall()
    rows = [r for r in rows if "tcx::" in r[0]]
    seq, cur = [], []
    for r in rows:
        if "k_first_acf" in r[0] and cur:
            seq.append(cur)
            cur = []
        cur.append(r)
    seq.append(cur)
    L = collections.Counter(len(s) for s in seq).most_common(1)[0][0]
    ev = [s for s in seq if len(s) == L]
    ev = ev[min(5, len(ev) // 2):]  # skip warm-up passes
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else sys.stdout
    print(f"{len(ev)} passes of {L} kernels; us: min p10 median p90 max", file=out)
    for i in range(L):
        d = sorted((s[i][2] - s[i][1]) / 1e3 for s in ev)
        p10, p90 = d[len(d) // 10], d[len(d) - 1 - len(d) // 10]
        print(f"{i:2d} {short(ev[0][i][0]):60s} grid={ev[0][i][3]:>8d} {d[0]:8.1f} {p10:8.1f} "
              f"{statistics.median(d):8.1f} {p90:8.1f} {d[-1]:8.1f}", file=out)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
