"""Cost of the control side of the loop: the device entry points against their host counterparts, the closed loop in three forms, and the
reset of a random 5 % of the envs.

(a) every device entry point (set_cmd_device, set_pd_target_device, set_xfrc_applied_device, get_joint_state_device) against its host
    counterpart on the C3 arm; set_xfrc_applied also on the C4 PR2 world (the widest rows: 6 nbody).
(b) the closed loop  get joint state -> ddq = -kd qvel -> set cmd -> step  on the C3 arm: through the host (numpy), on the device (one torch
    multiply between the two device calls, no synchronisation), and with the in-engine PD law (kp = 0: the same law, no call at all) as the
    ceiling; the last two also with one cohort (mjh_set_cohorts(1)): a full-range call between two steps then joins and forks no streams.
(c) reset of a random 5 % of the envs: reset_device with a mask, mjh_reset with the id list (one upload, one launch), mjh_reset one id per call
    (what a list cost before: one launch of the step kernel per id), and, with --parent-lib, the same list through another build of the
    library (an A/B build of the parent commit: mujoco_sim_amd/build.py, MJH_BUILD_DIR).

Every figure is event-timed on the engine's stream in windows of --reps calls (--host-reps for the host forms of (a), which wait for the
device in every call), each window closed by one synchronisation of the engines it used (it joins the cohort streams, which the closing
event alone would not wait for); the variants of a group alternate inside every trial; median and range of the trials' means.

    python tools/control_bench.py [--nenv 4096] [--reps 200] [--trials 7] [--parent-lib PATH] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")


def timed(variants, reps, trials, warmup, sync):
    """variants: name -> (callable, reps or None); -> name -> dict(us_median, us_min, us_max) per call"""
    import torch
    for f, _ in variants.values():
        for _ in range(warmup):
            f()
    sync()
    times = {k: [] for k in variants}
    for _ in range(trials):
        for k, (f, r) in variants.items():
            r = r or reps
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(r):
                f()
            sync()      # steps run on the cohorts' own streams: join them (and drain) before the closing event, once per window
            b.record(); b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / r)
    return {k: dict(us_median=float(np.median(t)), us_min=float(min(t)), us_max=float(max(t))) for k, t in times.items()}


def parent_reset(path, n, ids):
    """mjh_reset(ids) through another build of the library: its own model and engine of the C3 arm"""
    P = C.CDLL(path)
    P.mjh_scene_arm7.restype = C.c_void_p; P.mjh_scene_arm7.argtypes = [C.c_int]
    P.mjh_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p)]
    P.mjh_reset.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.c_int]
    P.mjh_step.argtypes = [C.c_void_p, C.c_int, C.c_int]; P.mjh_synchronize.argtypes = [C.c_void_p]; P.mjh_destroy.argtypes = [C.c_void_p]
    m = P.mjh_scene_arm7(1)
    h = C.c_void_p()
    assert P.mjh_create(m, n, 0, None, C.byref(h)) == 0
    P.mjh_step(h, 2, 0); P.mjh_synchronize(h)
    p = ids.ctypes.data_as(C.POINTER(C.c_int))
    return (lambda: P.mjh_reset(h, p, len(ids))), (lambda: (P.mjh_synchronize(h), P.mjh_destroy(h)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--host-reps", type=int, default=20, help="calls per timed window of the host forms of (a)")
    ap.add_argument("--trials", type=int, default=7, help="timed windows per variant (the variants alternate)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kd", type=float, default=0.75)
    ap.add_argument("--parent-lib", default=None, help="(c): another build of libmjhip.so, timed on the same id list")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mujoco_sim_amd as ms
    from mujoco_sim_amd import capi
    from mujoco_sim_amd.tables import load_model_tables

    dev = torch.device("cuda:0")
    n = args.nenv
    rng = np.random.default_rng(7)
    res = dict(nenv=n, reps=args.reps, host_reps=args.host_reps, trials=args.trials, device=torch.cuda.get_device_name(0))

    def f32(shape, s=1.0):
        a = rng.uniform(-s, s, shape).astype(np.float32)
        return a.astype(np.float64), torch.from_numpy(a).to(dev)

    # ---- (a) entry points, C3 arm
    m = ms.scene("arm7", 1)
    e = ms.Engine(m, n)
    e.set_state(qvel=rng.uniform(-0.5, 0.5, (n, m.nv)))
    e.set_pd_controller(0.0, args.kd); e.set_pd_controller(0.0, 0.0)      # targets exist, the law is off
    e.step(2)

    def sync():
        e.synchronize(); torch.cuda.synchronize()

    a64, a32 = f32((n, m.nv)); b64, b32 = f32((n, m.nv), 0.2); x64, x32 = f32((n, m.nbody, 6), 5.0)
    gq = torch.empty((n, m.nq), dtype=torch.float32, device=dev); gv = torch.empty((n, m.nv), dtype=torch.float32, device=dev)
    gf = torch.empty((n, m.nv), dtype=torch.float32, device=dev)
    e.set_xfrc_applied(x64)      # the first-use allocation is not part of a call's cost
    H = args.host_reps
    res["entry_points_c3_arm7"] = timed({
        "set_cmd_host": (lambda: e.set_cmd(a64, b64), H), "set_cmd_device": (lambda: e.set_cmd_device(a32, b32), None),
        "set_pd_target_host": (lambda: e.set_pd_target(a64), H), "set_pd_target_device": (lambda: e.set_pd_target_device(a32), None),
        "set_xfrc_applied_host": (lambda: e.set_xfrc_applied(x64), H), "set_xfrc_applied_device": (lambda: e.set_xfrc_applied_device(x32), None),
        "get_joint_state_host": (lambda: e.get_joint_state(), H), "get_joint_state_device": (lambda: e.get_joint_state_device(gq, gv, gf), None),
    }, args.reps, args.trials, args.warmup, sync)
    e.close()

    # ---- (a) the widest rows: xfrc_applied of the C4 PR2 world
    pr2 = os.path.join(GOLD, "robot_c4_pr2_world_objects_mesh.npz")
    if os.path.exists(pr2):
        mp = load_model_tables(pr2)[0]
        e = ms.Engine(mp, n)
        y64, y32 = f32((n, mp.nbody, 6), 5.0)
        e.set_xfrc_applied(y64)
        r = timed({"set_xfrc_applied_host": (lambda: e.set_xfrc_applied(y64), max(2, H // 4)),
                   "set_xfrc_applied_device": (lambda: e.set_xfrc_applied_device(y32), None)}, args.reps, args.trials, 2, sync)
        r["nbody"] = int(mp.nbody); r["floats_per_call"] = int(n * 6 * mp.nbody)
        res["xfrc_applied_c4_pr2"] = r
        e.close(); del y32

    # ---- (b) the closed loop, C3 arm: three engines in the same state
    kd = np.float32(args.kd)
    v0 = rng.uniform(-0.5, 0.5, (n, m.nv))
    eng = {}
    for k in ("host", "device", "in_engine_pd", "device_1c", "in_engine_pd_1c"):
        eng[k] = ms.Engine(m, n); eng[k].set_state(qvel=v0)
    for k in ("device_1c", "in_engine_pd_1c"):      # one cohort: a full-range call between two steps joins and forks no streams
        eng[k].set_cohorts(1)
    eng["in_engine_pd"].set_pd_controller(0.0, float(kd)); eng["in_engine_pd_1c"].set_pd_controller(0.0, float(kd))
    qv = torch.zeros((n, m.nv), dtype=torch.float32, device=dev)

    def loop_device_1c():
        eng["device_1c"].get_joint_state_device(qvel=qv)
        eng["device_1c"].set_cmd_device(qv * (-kd)); eng["device_1c"].step()

    def loop_host():
        v = eng["host"].get_joint_state()[1].astype(np.float32)
        eng["host"].set_cmd((v * (-kd)).astype(np.float64)); eng["host"].step()

    def loop_device():
        eng["device"].get_joint_state_device(qvel=qv)
        eng["device"].set_cmd_device(qv * (-kd)); eng["device"].step()

    def sync_all():
        for x in eng.values():
            x.synchronize()
        torch.cuda.synchronize()

    res["closed_loop_c3_arm7"] = timed({"host": (loop_host, max(2, args.reps // 4)), "device_torch": (loop_device, None),
                                        "in_engine_pd": (lambda: eng["in_engine_pd"].step(), None),
                                        "device_torch_one_cohort": (loop_device_1c, None),
                                        "in_engine_pd_one_cohort": (lambda: eng["in_engine_pd_1c"].step(), None)},
                                       args.reps, args.trials, args.warmup, sync_all)
    res["closed_loop_c3_arm7"]["cohorts_default"] = int(eng["device"].cohorts)
    for x in eng.values():
        x.close()

    # ---- (c) reset of a random 5 % of the envs
    e = ms.Engine(m, n); e.set_state(qvel=v0); e.step(2)
    ids = np.ascontiguousarray(np.sort(rng.choice(n, max(2, n // 20), replace=False)), dtype=np.int32)
    mask = torch.zeros(n, dtype=torch.uint8, device=dev); mask[torch.from_numpy(ids.astype(np.int64)).to(dev)] = 1
    lib, h = e.lib, e.h
    one = [capi.iptr(ids[i:i + 1]) for i in range(len(ids))]

    def single_ids():
        for p in one:
            lib.mjh_reset(h, p, 1)

    variants = {"reset_device_mask": (lambda: e.reset_device(mask), None), "mjh_reset_id_list": (lambda: lib.mjh_reset(h, capi.iptr(ids), len(ids)), None),
                "mjh_reset_one_id_per_call": (single_ids, max(2, args.reps // 10))}
    done = None
    if args.parent_lib:
        f, done = parent_reset(args.parent_lib, n, ids)
        variants["parent_lib_mjh_reset_id_list"] = (f, max(2, args.reps // 10))
    r = timed(variants, args.reps, args.trials, 2, sync)
    r["ids"] = int(len(ids))
    res["reset_5_percent_c3_arm7"] = r
    if done:
        done()
    e.close()

    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
