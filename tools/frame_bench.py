"""Time of one frame-state call: mjh_frame_state_device for 8 frames of every env, with and without the Jacobian, against the only route
to the same numbers without it — get_body_state + get_state to the host, then the numpy kinematics of tests/frame_ref.py.

Device route: the whole call (the position-stage launch plus mjh_frame_state_kernel), event-timed on the engine's stream in windows of
--reps calls; the two variants alternate inside every trial, the figures are the median and the range of the trials' means.
Host route: wall clock around get_body_state + get_state (they end in a synchronise), median over the trials; the numpy kinematics are
timed on the first --ref-envs envs and scaled to all of them (stated as such: python per env, it does not depend on the env).

Models: the C3 arm (ms.scene("arm7")) and the C4 PR2 world (tests/golden/robot_c4_pr2_world_objects_mesh.npz), random joint angles and
velocities.  Frames: the 8 deepest bodies; every second one relative to body 1, one in its own axes.

    python tools/frame_bench.py [--nenv 4096] [--reps 200] [--trials 7] [--out FILE]
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
GOLD = os.path.join(ROOT, "tests", "golden")


def models():
    import mujoco_sim_amd as ms
    from mujoco_sim_amd.tables import load_model_tables
    yield "c3_arm7", ms.scene("arm7", 1)
    yield "c4_pr2", load_model_tables(os.path.join(GOLD, "robot_c4_pr2_world_objects_mesh.npz"))[0]


def pick_frames(m):
    lev = m.array("body_level"); mocap = m.array("body_mocapid") if m.nmocap else -np.ones(m.nbody, int)
    deep = [int(b) for b in np.argsort(-lev, kind="stable") if mocap[b] < 0][:8]
    frames = []
    for k, b in enumerate(deep):
        frames.append(("body", b, dict(ref=("body", 1))) if k % 2 else ("body", b, dict(local=(k == 2))))
    return frames


def random_state(m, n, rng):
    from indep_dyn import Tree
    tr = Tree(m)
    q = np.tile(tr.q0, (n, 1)); v = rng.uniform(-1, 1, (n, m.nv))
    for j in range(tr.nj):
        a, t = tr.jq[j], tr.jtype[j]
        if t >= 2:
            lo, hi = tr.jrange[j] if tr.jlimited[j] and tr.jrange[j, 1] > tr.jrange[j, 0] else (-0.5, 0.5)
            q[:, a] = rng.uniform(lo, hi, n)
    return q, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=7, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--ref-envs", type=int, default=64, help="envs the numpy kinematics are timed on")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import frame_ref as fr
    import mujoco_sim_amd as ms

    dev = torch.device("cuda:0")
    n = args.nenv
    res = dict(nenv=n, nframe=8, reps=args.reps, trials=args.trials, device=torch.cuda.get_device_name(0), cases=[])
    rng = np.random.default_rng(7)
    for name, m in models():
        e = ms.Engine(m, n)
        q, v = random_state(m, n, rng)
        e.set_state(qpos=q, qvel=v, time=np.zeros(n), warmstart=np.zeros_like(v))
        frames = pick_frames(m)
        st = torch.empty((n, 8, 13), dtype=torch.float32, device=dev); jb = torch.empty((n, 8, 6, m.nv), dtype=torch.float32, device=dev)
        variants = {"state": lambda: e.frame_state_device(st.data_ptr(), None, frames),
                    "state_and_jacobian": lambda: e.frame_state_device(st.data_ptr(), jb.data_ptr(), frames)}
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
        # the host route: both copies, then the kinematics in numpy
        copies = []
        for _ in range(args.trials):
            e.synchronize()
            t0 = time.perf_counter()
            xp, xq = e.get_body_state(); _, qd, vd, _ = e.get_state()
            copies.append((time.perf_counter() - t0) * 1e3)
        R = fr.FrameRef(m)
        tup = [fr.frame_tuple(m, f) for f in frames]
        k = min(args.ref_envs, n)
        t0 = time.perf_counter()
        ref = [R.evaluate(qd[i], vd[i], tup) for i in range(k)]
        numpy_ms = (time.perf_counter() - t0) * 1e3 / k * n
        got = st.cpu().numpy().astype(np.float64)
        err = max(np.abs(got[i, :, 0:3] - ref[i]["pos"]).max() for i in range(k)), max(np.abs(got[i, :, 7:10] - ref[i]["linvel"]).max() for i in range(k))
        case = dict(model=name, nv=int(m.nv), nbody=int(m.nbody), frames=[list(t) for t in tup], variants={},
                    host_copies_ms_median=float(np.median(copies)), host_copies_ms_min=float(min(copies)), host_copies_ms_max=float(max(copies)),
                    host_numpy_ms_scaled=float(numpy_ms), host_numpy_envs_timed=k,
                    max_abs_pos_err_vs_numpy=float(err[0]), max_abs_linvel_err_vs_numpy=float(err[1]))
        for kk, ts in times.items():
            ts = np.array(ts)
            case["variants"][kk] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()))
        case["host_route_ms"] = case["host_copies_ms_median"] + case["host_numpy_ms_scaled"]
        res["cases"].append(case)
        del st, jb
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
