"""Does the assemble-only launch of the window chain run in one round?  Reads what a probe library (built with -DMJH_ASM_PROBE: step_kernel.h)
leaves in the stats slots: per env the start of its assemble workgroup on the 100 MHz wall clock, its duration, and the SIMD / CU / XCD it ran on.

    MJH_EXTRA_FLAGS=-DMJH_ASM_PROBE MJH_BUILD_DIR=build_exp/probe python -m mujoco_sim_amd.build
    MJHIP_LIB=build_exp/probe/libmjhip.so python bench.py --gpus 1 --steps 100 --warmup 20 --dump-outputs DIR
    python tools/assemble_rounds.py DIR [cohorts]

The slots hold the LAST step of the run: per cohort (env ranges as mjh_step splits them) one launch, in the timed window's steady state — the other
cohorts' chains run beside it, except for the cohort whose chain ends last (the table says which launch started when)."""
import os
import sys

import numpy as np

TICK_US = 0.01          # s_memrealtime: 100 MHz


def decode(stats):
    st = stats.astype(np.int64)
    start = st[:, 0] & 0x7FFFFFFF
    w = st[:, 2]
    return start, (w >> 13) & 0x3FFFF, w & 3, (w >> 2) & 0x7FF          # start tick, duration ticks, SIMD, CU key (CU, SH, SE of HW_ID | XCC_ID << 8)


def rounds(stats, cohorts=3, out=sys.stdout):
    start, dur, simd, cu = decode(stats)
    n = len(start)
    t_all = int(start.min())
    rows = []
    for g in range(cohorts):
        g0, g1 = n * g // cohorts, n * (g + 1) // cohorts
        s = (start[g0:g1] - start[g0:g1].min()) * TICK_US          # us behind the launch's first workgroup
        d = dur[g0:g1] * TICK_US
        end = s + d
        first = s < 1.0                                             # "the first instant": the workgroups of the first microsecond
        per_cu = np.bincount(cu[g0:g1][first], minlength=1)
        per_cu = per_cu[per_cu > 0]
        per_simd = np.bincount(((cu[g0:g1] << 2) | simd[g0:g1])[first]); per_simd = per_simd[per_simd > 0]
        rows.append(dict(cohort=g, wgs=g1 - g0, launch_start_us=(int(start[g0:g1].min()) - t_all) * TICK_US, within_5us=int((s < 5).sum()), later_20us=int((s > 20).sum()),
                         between=int(((s >= 5) & (s <= 20)).sum()), launch_us=float(end.max()), wg_us_mean=float(d.mean()), wg_us_median=float(np.median(d)), wg_us_max=float(d.max()),
                         late_wg_us_mean=float(d[s > 20].mean()) if (s > 20).any() else 0.0, cus=int(len(per_cu)), per_cu_mean=float(per_cu.mean()), per_cu_max=int(per_cu.max()),
                         per_cu_hist={int(k): int(v) for k, v in zip(*np.unique(per_cu, return_counts=True))}, per_simd_max=int(per_simd.max())))
    print("| cohort | launch starts at | workgroups | start < 5 us | 5 .. 20 us | start > 20 us | first to last end | workgroup mean / median / max | late ones' mean | CUs at the first us | per CU mean / max |", file=out)
    print("|---|---|---|---|---|---|---|---|---|---|---|", file=out)
    for r in rows:
        print(f"| {r['cohort']} | {r['launch_start_us']:.1f} us | {r['wgs']} | {r['within_5us']} | {r['between']} | {r['later_20us']} | {r['launch_us']:.1f} us | "
              f"{r['wg_us_mean']:.1f} / {r['wg_us_median']:.1f} / {r['wg_us_max']:.1f} us | {r['late_wg_us_mean']:.1f} us | {r['cus']} | {r['per_cu_mean']:.2f} / {r['per_cu_max']} |", file=out)
    for r in rows:
        print(f"cohort {r['cohort']}: workgroups per CU in the first microsecond (count: CUs) {r['per_cu_hist']}, most on one SIMD {r['per_simd_max']}", file=out)
    return rows


if __name__ == "__main__":
    d = sys.argv[1]
    rounds(np.load(os.path.join(d, "stats.npy")), int(sys.argv[2]) if len(sys.argv) > 2 else 3)
