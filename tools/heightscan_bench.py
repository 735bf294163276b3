"""Time of a height scan per env: mjh_heightscan_device with the tile cull on and off, against mjh_ray_device with per_env = 1 fed the
same rays — the only route a caller had before the height-scan kernel.  The ray route's rays are built once on the host (fp64, from
the device's own site poses, rounded to fp32) and uploaded once: what that route costs a caller on every call — building and
uploading n * width * height origins and directions — is NOT in its figures.  Every route is the whole call: the position-stage
launch plus its kernel, event-timed on the engine's stream.  The routes alternate inside every trial, so a drift of the machine hits
all of them; the figures are the median and the range of the trials' means.

Scenes: S24 (rebuilt from the scene's own tables with a sensor site above the pen, per-env sizes and poses, settled), the 107-geom
tetrahedron field of tests/ray_mesh_ref.py in mesh mode 1 with the sensor above it, and the height-field terrain C of tests/ray_ref.py
with six free bodies on it.  Grids: 16 x 16 at 0.1 m and 64 x 64 at 0.05 m, YAW alignment, cast from 1 m above the site.
kept_per_tile: the mean number of geoms a tile stages with the cull on (fp64 restatement of the cylinder test on env 0's poses), of
the geoms a ray may see.

    python tools/heightscan_bench.py [--nenv 4096] [--reps 100] [--trials 5] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

S24_SENSOR = ((0.05, -0.1, 0.9), (1.0, 0.0, 0.0, 0.0))
TETRA_SENSOR = ((0.0, 0.225, 2.0), (0.9553364891256060, 0.0, 0.0, 0.2955202066613396))      # yawed 0.6 rad
TERRAIN_SENSOR = ((0.2, -0.1, 1.5), (0.9800665778412416, 0.0, 0.0, 0.1986693307950612))     # yawed 0.4 rad
GRIDS = {
    "16x16 at 0.1 m": (16, 16, (0.1, 0.1), (0.0, 0.0), 1.0),
    "64x64 at 0.05 m": (64, 64, (0.05, 0.05), (0.0, 0.0), 1.0),
}


def add_sensor(sensor):
    def extra(lib, b):
        from helpers import D
        assert lib.mjh_builder_add_site(b, b"scanner", 0, D(*sensor[0]), D(*sensor[1])) == 0, lib.mjh_last_error()
    return extra


def terrain_model(lib):
    """terrain C (17 x 33 nodes, 8 m x 4 m) with six free bodies — spheres, boxes, a capsule — standing on or above it"""
    import mujoco_sim_amd as ms
    import ray_ref as rr
    from helpers import D, set_opt
    nrow, ncol, size, elev = rr.terrain("C")
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    h = lib.mjh_builder_add_hfield(b, b"terrain", nrow, ncol, D(*size), (C.c_double * elev.size)(*elev.ravel()))
    assert h >= 0
    assert lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(0, 0, 0), None, None, -1, -1, -1) >= 0
    items = [(rr.SPHERE, (0.2, 0, 0), (0.5, 0.3, 0.8)), (rr.BOX, (0.25, 0.15, 0.1), (-0.6, -0.4, 0.75)), (rr.CAPSULE, (0.1, 0.3, 0), (1.1, -0.7, 0.9)),
             (rr.SPHERE, (0.15, 0, 0), (-1.2, 0.6, 0.8)), (rr.BOX, (0.2, 0.2, 0.2), (0.1, -1.0, 0.85)), (rr.ELLIPSOID, (0.3, 0.2, 0.1), (-0.3, 0.9, 0.8))]
    for k, (t, s, pos) in enumerate(items):
        bd = lib.mjh_builder_add_body(b, b"obj%d" % k, 0, D(*pos), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_geom(b, b"og%d" % k, bd, t, D(*s), None, None, None, -1, -1, -1, -1) >= 0
    add_sensor(TERRAIN_SENSOR)(lib, b)
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m


def site_poses(e, m, n):
    """(o [n, 3], S [n, 3, 3]) of site 0 in every env, from the device's own body poses"""
    import ray_ref as rr
    xp, xq = e.get_body_state(0, n)
    b = int(m.array("site_bodyid")[0])
    Rb = np.array([rr.quat2mat(q).reshape(3, 3) for q in xq[:, b]])
    return xp[:, b] + Rb @ m.array("site_pos").reshape(-1, 3)[0], Rb @ rr.quat2mat(m.array("site_quat").reshape(-1, 4)[0]).reshape(3, 3)


def kept_per_tile(e, m, pose, grid):
    """mean over the tiles of the number of geoms staged with the cull on: the never-culled planes and height fields plus the bounded
    geoms whose bounding sphere touches the tile's cylinder (fp64, env 0, every geom of the table taken as visible)"""
    import heightscan_ref as hr
    import ray_ref as rr
    width, height = grid[:2]
    th, tw = hr.tile_shape(height)
    G = hr.grid_frame(pose[1], "yaw")
    x, y = hr.cells(grid)
    gp, _ = e.get_geom_state(0, 1)
    types, size = m.array("geom_type"), m.array("geom_size").reshape(-1, 3)
    mesh_r = [np.linalg.norm(v, axis=1).max() for v in __import__("ray_mesh_ref").model_mesh_verts(m)] if (types == rr.MESH).any() else []
    did = m.array("geom_dataid")
    r = np.array([mesh_r[did[g]] if types[g] == rr.MESH else rr.rbound(int(types[g]), size[g]) for g in range(len(types))])
    bounded = (types >= rr.SPHERE) & (types != rr.HFIELD)
    u = -G[:, 2]
    counts = []
    for i0 in range(0, height, th):
        for j0 in range(0, width, tw):
            xs, ys = x[j0:j0 + tw], y[i0:i0 + th]
            a = pose[0] + G[:, 0] * 0.5 * (xs[0] + xs[-1]) + G[:, 1] * 0.5 * (ys[0] + ys[-1]) + G[:, 2] * grid[4]
            radius = 0.5 * np.hypot(xs[-1] - xs[0], ys[-1] - ys[0])
            d = gp[0] - a; h = d @ u; q = np.linalg.norm(d - h[:, None] * u, axis=1)
            counts.append(int((~bounded | ((h >= -r) & (q <= radius + r))).sum()))
    return float(np.mean(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=5, help="timed windows per route (the routes alternate)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=200, help="S24: steps before the scans")
    ap.add_argument("--scenes", nargs="+", default=["s24", "tetra", "terrain"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import depth_bench
    import heightscan_ref as hr
    import mujoco_sim_amd as ms
    from mujoco_sim_amd import capi

    lib = capi.load()
    dev = torch.device("cuda:0")
    n = args.nenv
    res = dict(nenv=n, reps=args.reps, trials=args.trials, device=torch.cuda.get_device_name(0), align="yaw",
               ray_route_note="rays built once on the host and uploaded once; the per-call cost of building and uploading them is not counted", cases=[])
    for name in args.scenes:
        if name == "s24":
            m, s = depth_bench.s24_with_camera(lib, extra=add_sensor(S24_SENSOR))
            e = ms.Engine(m, n)
            t = s.s24_randomize(0, n)
            for k in ["geom_size", "geom_rbound", "body_mass", "body_inertia", "body_invweight0", "dof_invweight0"]:
                e.set_env_param(k, t[k])
            e.set_initial_qpos(t["qpos"]); e.reset()
            e.step(args.settle); e.synchronize()
        elif name == "tetra":
            m = depth_bench.tetra_with_camera(lib, extra=add_sensor(TETRA_SENSOR))
            e = ms.Engine(m, n)
            e.ray_mesh_mode = 1
        else:
            m = terrain_model(lib)
            e = ms.Engine(m, n)
        o, S = site_poses(e, m, n)
        for gname, grid in GRIDS.items():
            W, H = grid[:2]
            kw = hr.kwargs(grid)
            # the ray route's input: every env's rays in the world frame, fp64 from the device's poses, rounded to fp32, uploaded once
            tp = torch.empty((n, W * H, 3), dtype=torch.float32, device=dev); tv = torch.empty((n, W * H, 3), dtype=torch.float32, device=dev)
            if (o == o[0]).all() and (S == S[0]).all():      # (a sensor on the world body: one pose)
                P, V = hr.rays64((o[0], S[0]), grid, "yaw")
                tp.copy_(torch.tensor(P, dtype=torch.float32).to(dev).expand(n, -1, -1)); tv.copy_(torch.tensor(V, dtype=torch.float32).to(dev).expand(n, -1, -1))
            else:
                for k in range(n):
                    P, V = hr.rays64((o[k], S[k]), grid, "yaw")
                    tp[k].copy_(torch.tensor(P, dtype=torch.float32)); tv[k].copy_(torch.tensor(V, dtype=torch.float32))
            routes = {
                "heightscan_cull1": lambda d, g: e.height_scan_device(d.data_ptr(), g.data_ptr(), None, 0, cull=1, **kw),
                "heightscan_cull0": lambda d, g: e.height_scan_device(d.data_ptr(), g.data_ptr(), None, 0, cull=0, **kw),
                "ray_device": lambda d, g: e.ray_device(tp.data_ptr(), tv.data_ptr(), d.data_ptr(), g.data_ptr(), W * H, per_env=True),
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
            d1, g1 = img["heightscan_cull1"]; d0, g0 = img["heightscan_cull0"]; dr, gr = img["ray_device"]
            same = g1 == gr
            case = dict(scene=name, grid=gname, width=W, height=H, spacing=grid[2][0], ngeom=int(m.c.ngeom), mesh_mode=e.ray_mesh_mode,
                        hit_share=float((g1 >= 0).mean()), geoms_seen=int(len(np.unique(g1[g1 >= 0]))), kept_per_tile=kept_per_tile(e, m, (o[0], S[0]), grid),
                        cull_bitwise_equal=bool(np.array_equal(d1.view(np.uint32), d0.view(np.uint32)) and np.array_equal(g1, g0)),
                        ray_route_same_geom_share=float(same.mean()),
                        ray_route_max_abs_diff_where_same_geom=float(np.abs(d1 - dr)[same & (g1 >= 0)].max(initial=0.0)), routes={})
            for r in routes:
                ts = np.array(times[r])
                case["routes"][r] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                                         rays_per_s=n * W * H / (float(np.median(ts)) * 1e-3))
            med = {r: case["routes"][r]["ms_median"] for r in routes}
            case["cull1_over_cull0"] = med["heightscan_cull1"] / med["heightscan_cull0"]
            case["cull1_over_ray_device"] = med["heightscan_cull1"] / med["ray_device"]
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
