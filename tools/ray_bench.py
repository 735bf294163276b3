"""Throughput of batched ray casting on S24: mjh_ray_device (position-stage launch + mjh_ray_kernel, event-timed on the engine's
stream) against the host route a caller had before it — mjh_get_geom_state of every env plus the numpy loop of tests/ray_ref.py —
and against the position-stage launch alone (approximated by a one-ray call: the same launch chain with an almost empty ray kernel).

    python tools/ray_bench.py [--nenv 4096] [--nray 64 360] [--reps 50] [--host-envs 4096] [--out FILE]
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


def scan(nray):
    """a planar laser fan from above the pen's centre, pitched 35 degrees down"""
    a = np.linspace(0.0, 2 * np.pi, nray, endpoint=False)
    c = np.cos(np.radians(35.0))
    V = np.stack([c * np.cos(a), c * np.sin(a), np.full(nray, -np.sin(np.radians(35.0)))], axis=1)
    return np.tile([0.0, 0.0, 1.2], (nray, 1)), V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--nray", type=int, nargs="+", default=[64, 360])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--settle", type=int, default=200, help="steps before the scans")
    ap.add_argument("--host-envs", type=int, default=4096, help="envs the host loop intersects (its time is scaled to --nenv)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mujoco_sim_amd as ms
    import ray_ref as rr

    m = ms.scene("s24")
    e = ms.Engine(m, args.nenv)
    tab = e.load_s24()
    e.step(args.settle); e.synchronize()
    dev = torch.device("cuda:0")
    res = dict(scene="s24", nenv=args.nenv, reps=args.reps, device=torch.cuda.get_device_name(0), cases=[])

    def time_device(nray):
        P, V = scan(nray)
        tp = torch.tensor(P, dtype=torch.float32, device=dev); tv = torch.tensor(V, dtype=torch.float32, device=dev)
        td = torch.empty((args.nenv, nray), dtype=torch.float32, device=dev); tg = torch.empty((args.nenv, nray), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        for _ in range(args.warmup):
            e.ray_device(tp.data_ptr(), tv.data_ptr(), td.data_ptr(), tg.data_ptr(), nray)
        e.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.reps):
            e.ray_device(tp.data_ptr(), tv.data_ptr(), td.data_ptr(), tg.data_ptr(), nray)
        b.record(); b.synchronize()
        return a.elapsed_time(b) / args.reps, td.cpu().numpy(), tg.cpu().numpy()

    fk_ms, _, _ = time_device(1)
    res["position_stage_plus_one_ray_ms"] = fk_ms
    for nray in args.nray:
        ms_dev, dist, gid = time_device(nray)
        P, V = scan(nray)
        # the host route: every geom pose to the host, then the numpy reference env by env
        t0 = time.perf_counter()
        gp, gm = e.get_geom_state()
        t1 = time.perf_counter()
        nh = min(args.host_envs, args.nenv)
        types = m.array("geom_type")
        worst = 0.0
        for i in range(nh):
            sc = rr.scene_from_device(gp[i], gm[i], tab["geom_size"][i], types)
            d, g = rr.cast(P, V, sc)
            same = g == gid[i]
            worst = max(worst, float(np.abs(d - dist[i])[same & (g >= 0)].max(initial=0.0)))
        t2 = time.perf_counter()
        host_ms = (t1 - t0) * 1e3 + (t2 - t1) * 1e3 * args.nenv / nh
        res["cases"].append(dict(nray=nray, ray_device_ms=ms_dev, rays_per_s=args.nenv * nray / (ms_dev * 1e-3),
                                 get_geom_state_ms=(t1 - t0) * 1e3, host_loop_ms=(t2 - t1) * 1e3 * args.nenv / nh, host_envs_timed=nh,
                                 host_total_ms=host_ms, speedup=host_ms / ms_dev, hit_share=float((gid >= 0).mean()),
                                 max_abs_diff_where_same_geom=worst))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
