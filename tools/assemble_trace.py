"""The window chain's two launches in a rocprofv3 kernel trace (rocpd .db, first found under the directory) of a plain S24 bench line: mean / median /
max of the last N launches of the assemble-only instance and of the window kernel (N = steps x cohorts: the timed window), of the launch-order sorts among them, and the cohort-step —
the span of those launches over the steps.     python tools/assemble_trace.py <dir> [steps] [cohorts]"""
import glob
import os
import sqlite3
import statistics
import sys

d = sys.argv[1]; steps = int(sys.argv[2]) if len(sys.argv) > 2 else 300; cohorts = int(sys.argv[3]) if len(sys.argv) > 3 else 3
f = glob.glob(os.path.join(d, "**", "*.db"), recursive=True)
con = sqlite3.connect(f[0])
rows = con.execute("select k.name, k.start, k.end from kernels k order by k.start").fetchall()
n = steps * cohorts
asm = [r for r in rows if "mjh_step_kernel" in r[0]][-n:]
win = [r for r in rows if "mjh_window_kernel" in r[0]][-n:]
print("| kernel | launches | mean (us) | median (us) | max (us) |")
print("|---|---|---|---|---|")
srt = [r for r in rows if "mjh_order_kernel" in r[0] and r[1] >= asm[0][1]]        # the launch-order sorts inside the timed window (every 32nd step and cohort)
for lst in (asm, win) + ((srt,) if srt else ()):
    us = [(e - s) / 1e3 for _, s, e in lst]
    print(f"| `{lst[0][0].split('(')[0].replace('void ', '')}` | {len(us)} | {statistics.mean(us):.1f} | {statistics.median(us):.1f} | {max(us):.1f} |")
t0 = min(r[1] for r in asm + win); t1 = max(r[2] for r in asm + win)
print(f"\nwindow: {(t1 - t0) / 1e3:.0f} us for {len(asm)} assemble + {len(win)} window launches on {cohorts} streams: **{(t1 - t0) / 1e3 / steps:.1f} us per cohort-step**")
