"""Time of a lidar scan per env: mjh_scan_device with the tile cull on and off, against mjh_ray_device fed the same beams in the site's
frame (uploaded once) — the only route a caller had before the scan kernel.  Every route is the whole call: the position-stage launch
plus its kernel, event-timed on the engine's stream.  The routes alternate inside every trial, so a drift of the machine hits all of
them; the figures are the median and the range of the trials' means.

Scenes: S24 (rebuilt from the scene's own tables with a sensor site above the pen, per-env sizes and poses, settled) and the 107-geom
tetrahedron field of tests/ray_mesh_ref.py in mesh mode 1, the sensor among the tetrahedra.  Patterns: a 16 x 1024 full turn and a
1 x 1081 planar scan.  kept_per_tile: the mean number of geoms a tile stages with the cull on (fp64 restatement of the cone test on
env 0's poses), of the geoms a ray may see.

    python tools/scan_bench.py [--nenv 4096] [--reps 100] [--trials 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

DEG = np.pi / 180
S24_SENSOR = ((0.05, -0.1, 0.9), (1.0, 0.0, 0.0, 0.0))
TETRA_SENSOR = ((0.0, 0.225, 0.75), (1.0, 0.0, 0.0, 0.0))
PATTERNS = {
    "full turn 16x1024": (1024, 16, -np.pi, 2 * np.pi / 1024, (-30.0 * DEG, 2.0 * DEG)),
    "planar 1x1081": (1081, 1, -135.0 * DEG, 0.25 * DEG, (-0.1, 0.0)),
}


def add_sensor(sensor):
    def extra(lib, b):
        from helpers import D
        assert lib.mjh_builder_add_site(b, b"lidar", 0, D(*sensor[0]), D(*sensor[1])) == 0, lib.mjh_last_error()
    return extra


def kept_per_tile(e, m, sensor, pattern):
    """mean over the tiles of the number of geoms staged with the cull on: the never-culled planes and height fields plus the bounded
    geoms whose bounding sphere touches the tile's cone (fp64, env 0, every geom of the table taken as visible)"""
    import ray_ref as rr
    import scan_ref as sr
    width, height = pattern[:2]
    th, tw = sr.tile_shape(height)
    Dn = sr.beams64(pattern)
    gp, _ = e.get_geom_state(0, 1)
    types, size = m.array("geom_type"), m.array("geom_size").reshape(-1, 3)
    mesh_r = [np.linalg.norm(v, axis=1).max() for v in __import__("ray_mesh_ref").model_mesh_verts(m)] if (types == rr.MESH).any() else []
    did = m.array("geom_dataid")
    c = gp[0] - np.asarray(sensor[0]); r = np.array([mesh_r[did[g]] if types[g] == rr.MESH else rr.rbound(int(types[g]), size[g]) for g in range(len(types))])
    bounded = (types >= rr.SPHERE) & (types != rr.HFIELD)
    counts = []
    for i0 in range(0, height, th):
        for j0 in range(0, width, tw):
            ni, nj = min(th, height - i0), min(tw, width - j0)
            rows = Dn[i0:i0 + ni, j0, 2]; lo, hi = i0 + int(np.argmin(rows)), i0 + int(np.argmax(rows))
            corners = np.array([Dn[a, b] for a in (lo, hi) for b in (j0, j0 + nj - 1)])
            axis = corners.sum(axis=0); nrm = np.linalg.norm(axis)
            keep = np.ones(len(types), bool)
            if (nj - 1) * abs(pattern[3]) <= np.pi and nrm > 1e-3 and (corners @ axis / nrm).min() > 0:
                axis /= nrm; cosA = (corners @ axis).min(); sinA = np.sqrt(max(0.0, 1 - cosA * cosA))
                h = c @ axis; q = np.linalg.norm(np.cross(c, axis), axis=1)
                keep = ~bounded | (np.einsum("ij,ij->i", c, c) <= r * r) | ((h >= -r) & (q * cosA - h * sinA <= r))
            counts.append(int(keep.sum()))
    return float(np.mean(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=5, help="timed windows per route (the routes alternate)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=200, help="S24: steps before the scans")
    ap.add_argument("--scenes", nargs="+", default=["s24", "tetra"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import depth_bench
    import mujoco_sim_amd as ms
    import scan_ref as sr
    from mujoco_sim_amd import capi

    lib = capi.load()
    dev = torch.device("cuda:0")
    n = args.nenv
    res = dict(nenv=n, reps=args.reps, trials=args.trials, device=torch.cuda.get_device_name(0), cases=[])
    for name in args.scenes:
        if name == "s24":
            sensor = S24_SENSOR
            m, s = depth_bench.s24_with_camera(lib, extra=add_sensor(sensor))
            e = ms.Engine(m, n)
            t = s.s24_randomize(0, n)
            for k in ["geom_size", "geom_rbound", "body_mass", "body_inertia", "body_invweight0", "dof_invweight0"]:
                e.set_env_param(k, t[k])
            e.set_initial_qpos(t["qpos"]); e.reset()
            e.step(args.settle); e.synchronize()
        else:
            sensor = TETRA_SENSOR
            m = depth_bench.tetra_with_camera(lib, extra=add_sensor(sensor))
            e = ms.Engine(m, n)
            e.ray_mesh_mode = 1
        for pname, pattern in PATTERNS.items():
            W, H = pattern[:2]
            kw = sr.scan_kwargs(pattern)
            Ds = sr.beams64(pattern).reshape(-1, 3)
            tp = torch.zeros((W * H, 3), dtype=torch.float32, device=dev); tv = torch.tensor(Ds, dtype=torch.float32, device=dev)
            routes = {
                "scan_cull1": lambda d, g: e.scan_device(d.data_ptr(), g.data_ptr(), None, 0, cull=1, **kw),
                "scan_cull0": lambda d, g: e.scan_device(d.data_ptr(), g.data_ptr(), None, 0, cull=0, **kw),
                "ray_device": lambda d, g: e.ray_device(tp.data_ptr(), tv.data_ptr(), d.data_ptr(), g.data_ptr(), W * H, site=0),
            }
            out = {r: (torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.int32, device=dev)) for r in routes}
            torch.cuda.synchronize()
            for r, f in routes.items():
                for _ in range(args.warmup):
                    f(*out[r])
            e.synchronize()
            times = {r: [] for r in routes}
            for _ in range(args.trials):
                for r, f in routes.items():
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(args.reps):
                        f(*out[r])
                    b.record(); b.synchronize()
                    times[r].append(a.elapsed_time(b) / args.reps)
            img = {r: (out[r][0].cpu().numpy(), out[r][1].cpu().numpy()) for r in routes}
            d1, g1 = img["scan_cull1"]; d0, g0 = img["scan_cull0"]; dr, gr = img["ray_device"]
            same = g1 == gr
            case = dict(scene=name, pattern=pname, width=W, height=H, ngeom=int(m.c.ngeom), mesh_mode=e.ray_mesh_mode, hit_share=float((g1 >= 0).mean()),
                        geoms_seen=int(len(np.unique(g1[g1 >= 0]))), kept_per_tile=kept_per_tile(e, m, sensor, pattern),
                        cull_bitwise_equal=bool(np.array_equal(d1.view(np.uint32), d0.view(np.uint32)) and np.array_equal(g1, g0)),
                        ray_route_same_geom_share=float(same.mean()),
                        ray_route_max_abs_diff_where_same_geom=float(np.abs(d1 - dr)[same & (g1 >= 0)].max(initial=0.0)), routes={})
            for r in routes:
                ts = np.array(times[r])
                case["routes"][r] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                                         beams_per_s=n * W * H / (float(np.median(ts)) * 1e-3))
            med = {r: case["routes"][r]["ms_median"] for r in routes}
            case["cull1_over_cull0"] = med["scan_cull1"] / med["scan_cull0"]
            case["cull1_over_ray_device"] = med["scan_cull1"] / med["ray_device"]
            res["cases"].append(case)
            del out, tp, tv
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
