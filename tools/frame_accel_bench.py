"""Time of one frame-acceleration call: mjh_frame_accel_device for 8 frames of every env, with and without the bias output, beside
mjh_frame_state_device on the same selection and the only route to the same numbers without the call — get_state and get_field("qacc")
to the host, then the numpy kinematics of tests/frame_acc_ref.py.

Device route: the whole call (the position-stage launch plus the kernel), event-timed on the engine's stream in windows of --reps calls;
the variants alternate inside every trial, the figures are the median and the range of the trials' means.
Host route: wall clock around get_state + get_field (they end in a synchronise), median over the trials; the numpy kinematics are timed on
the first --ref-envs envs and scaled to all of them (stated as such: python per env, it does not depend on the env).

Models: the C3 arm (ms.scene("arm7")) and the C4 PR2 world (tests/golden/robot_c4_pr2_world_objects_mesh.npz), random joint angles,
velocities and qacc (through the warm start).  Frames: the 8 deepest bodies, alternately LOCAL | PROPER (an accelerometer) and plain.

    python tools/frame_accel_bench.py [--nenv 4096] [--reps 200] [--trials 7] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def pick_frames(m):
    lev = m.array("body_level"); mocap = m.array("body_mocapid") if m.nmocap else -np.ones(m.nbody, int)
    deep = [int(b) for b in np.argsort(-lev, kind="stable") if mocap[b] < 0][:8]
    return [("body", b) if k % 2 else ("body", b, dict(local=True, proper=True)) for k, b in enumerate(deep)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=7, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-envs", type=int, default=16, help="envs the numpy kinematics are timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import frame_acc_ref as far
    import mujoco_sim_amd as ms
    from frame_bench import models, random_state

    dev = torch.device("cuda:0")
    n = args.nenv
    res = dict(nenv=n, nframe=8, reps=args.reps, trials=args.trials, device=torch.cuda.get_device_name(0), cases=[])
    rng = np.random.default_rng(7)
    for name, m in models():
        e = ms.Engine(m, n)
        q, v = random_state(m, n, rng)
        e.set_state(qpos=q, qvel=v, time=np.zeros(n), warmstart=rng.uniform(-5, 5, v.shape))
        frames = pick_frames(m)
        same = [f[:2] for f in frames]      # the selection as frame_state takes it
        ac = torch.empty((n, 8, 6), dtype=torch.float32, device=dev); bs = torch.empty((n, 8, 6), dtype=torch.float32, device=dev)
        st = torch.empty((n, 8, 13), dtype=torch.float32, device=dev)
        variants = {"accel": lambda: e.frame_accel_device(ac.data_ptr(), None, frames),
                    "accel_and_bias": lambda: e.frame_accel_device(ac.data_ptr(), bs.data_ptr(), frames),
                    "frame_state": lambda: e.frame_state_device(st.data_ptr(), None, same)}
        for f in variants.values():
            for _ in range(args.warmup):
                f()
        e.synchronize(); torch.cuda.synchronize()
        times = {k: [] for k in variants}
        for _ in range(args.trials):
            for k, f in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    f()
                b.record(); b.synchronize()
                times[k].append(a.elapsed_time(b) / args.reps)
        # the host route: the copies, then the kinematics in numpy
        copies = []
        for _ in range(args.trials):
            e.synchronize()
            t0 = time.perf_counter()
            _, qd, vd, _ = e.get_state(); ad = e.get_field("qacc")
            copies.append((time.perf_counter() - t0) * 1e3)
        R = far.FrameAccRef(m)
        tup = [far.accel_tuple(m, f) for f in frames]
        k = min(args.ref_envs, n)
        t0 = time.perf_counter()
        ref = [R.evaluate_acc(qd[i], vd[i], ad[i], tup) for i in range(k)]
        numpy_ms = (time.perf_counter() - t0) * 1e3 / k * n
        got = ac.cpu().numpy().astype(np.float64)
        err = max((np.abs(got[i, :, 0:3] - ref[i]["linacc"]) / np.maximum(1.0, ref[i]["s"][:, 0:3])).max() for i in range(k))
        case = dict(model=name, nv=int(m.nv), nbody=int(m.nbody), frames=[list(t) for t in tup], variants={},
                    host_copies_ms_median=float(np.median(copies)), host_copies_ms_min=float(min(copies)), host_copies_ms_max=float(max(copies)),
                    host_numpy_ms_scaled=float(numpy_ms), host_numpy_envs_timed=k, max_linacc_err_over_scale_vs_numpy=float(err))
        for kk, ts in times.items():
            ts = np.array(ts)
            case["variants"][kk] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()))
        case["host_route_ms"] = case["host_copies_ms_median"] + case["host_numpy_ms_scaled"]
        res["cases"].append(case)
        del ac, bs, st
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
