"""What the contact report costs, and what the per-body contact force costs on top of it.

  env-steps/s of bench.py's own workloads (default S24 and C4) with the report off and on: the same command, the same process layout,
  only MJH_CONTACT_REPORT differs (the switch of engines created afterwards follows it).  The two alternate inside every trial, so a
  drift of the machine hits both; the figures are the median and the range over the trials.

  the body-sum launch (mjh_body_contact_force_device, 4 bodies on --nenv envs of a settled report-on S24): event-timed on the engine's
  stream, the selection table already on the device.

    python tools/contact_bench.py [--configs s24 c4] [--steps 300] [--warmup 50] [--trials 3] [--nenv 4096] [--reps 200] [--out FILE]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_line(config, steps, warmup, report):
    env = dict(os.environ); env["MJH_CONTACT_REPORT"] = "1" if report else "0"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--no-cpu-baseline", "--no-second-window", "--no-extra-configs"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py --config {config} (report {int(report)}): rc {r.returncode}: {r.stderr[-800:]}")
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"]


def body_sum_ms(nenv, reps, trials, settle):
    import torch

    import mujoco_sim_amd as ms

    m = ms.scene("s24")
    e = ms.Engine(m, nenv, contact_report=True)
    e.load_s24(); e.step(settle); e.synchronize()
    bodies = [b for b in range(1, m.nbody) if m.array("body_dofnum")[b] == 6][:4]
    f = torch.empty((nenv, len(bodies), 3), dtype=torch.float32, device="cuda:0"); c = torch.empty((nenv, len(bodies)), dtype=torch.int32, device="cuda:0")
    for _ in range(3):
        e.body_contact_force_device(f.data_ptr(), c.data_ptr(), bodies)
    e.synchronize()
    ts = []
    for _ in range(trials):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            e.body_contact_force_device(f.data_ptr(), c.data_ptr(), bodies)
        b.record(); b.synchronize()
        ts.append(a.elapsed_time(b) / reps)
    ncon = float(e.contact_forces()["ncon"].mean())
    out = dict(nenv=nenv, bodies=len(bodies), reps=reps, ms_median=float(np.median(ts)), ms_min=float(min(ts)), ms_max=float(max(ts)),
               mean_ncon=ncon, mean_contacts_per_sum=float(c.cpu().numpy().mean()))
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="*", default=["s24", "c4"])
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--trials", type=int, default=3)
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--settle", type=int, default=400)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = dict(steps=args.steps, warmup=args.warmup, trials=args.trials, configs={})
    for cfg in args.configs:
        vals = {0: [], 1: []}
        for _ in range(args.trials):
            for rep in (0, 1):
                vals[rep].append(bench_line(cfg, args.steps, args.warmup, bool(rep)))
        row = {("report_on" if rep else "report_off"): dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for rep, v in vals.items()}
        row["on_over_off"] = row["report_on"]["median"] / row["report_off"]["median"]
        res["configs"][cfg] = row
    res["body_sum"] = body_sum_ms(args.nenv, args.reps, max(args.trials, 3), args.settle)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
