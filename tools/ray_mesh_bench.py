"""Throughput of batched ray casting on the PR2 world model (the world file's floor + PR2 with its 18 mesh assets, 37 mesh geoms of 56
geoms) in mesh mode 0 (mesh geoms invisible) and mesh mode 1 (hit as their convex hulls): the same fan, mjh_ray_device event-timed
on the engine's stream as tools/ray_bench.py does, at qpos0.  The model is compiled by the MJCF loader from the bundled model files
(tests/refmodels.py).

    python tools/ray_mesh_bench.py [--nenv 1024] [--nray 128 360] [--reps 50] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def fan(nray):
    """a scanner 2 m in front of the robot at chest height looking back at it: nray beams on a raster of +-13 degrees azimuth and
    -27 .. +8 degrees elevation, 16 columns"""
    ncol = min(16, nray)
    nrow = (nray + ncol - 1) // ncol
    az = np.deg2rad(np.linspace(-13.0, 13.0, ncol) + 0.37)
    el = np.deg2rad(np.linspace(-27.0, 8.0, max(nrow, 2))[:nrow] + 0.21)
    A, E = np.meshgrid(az, el)
    V = np.stack([-np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)[:nray]
    return np.tile([2.0, 0.0, 1.0], (nray, 1)), V


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=1024)
    ap.add_argument("--nray", type=int, nargs="+", default=[128, 360])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mujoco_sim_amd as ms
    import ray_mesh_ref as rm
    from mujoco_sim_amd import capi

    lib = capi.load()
    m = rm.load_robot(lib, "pr2", world=True)
    types = m.array("geom_type")
    e = ms.Engine(m, args.nenv)
    dev = torch.device("cuda:0")
    res = dict(scene="pr2_world_mesh", nenv=args.nenv, reps=args.reps, ngeom=int(m.ngeom), mesh_geoms=int((types == 7).sum()),
               mesh_planes=int(m.c.nmeshplane), device=torch.cuda.get_device_name(0), cases=[])

    def time_device(nray):
        P, V = fan(nray)
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
        return a.elapsed_time(b) / args.reps, tg.cpu().numpy()

    for mode in (0, 1):
        e.ray_mesh_mode = mode
        fk_ms, _ = time_device(1)
        for nray in args.nray:
            ms_dev, gid = time_device(nray)
            hit = gid[0] >= 0
            res["cases"].append(dict(mesh_mode=mode, nray=nray, ray_device_ms=ms_dev, position_stage_plus_one_ray_ms=fk_ms,
                                     rays_per_s=args.nenv * nray / (ms_dev * 1e-3), hit_share=float(hit.mean()),
                                     mesh_hit_share=float((types[gid[0][hit]] == 7).mean()) if hit.any() else 0.0))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
