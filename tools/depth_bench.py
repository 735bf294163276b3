"""Time of a depth image per env: mjh_depth_device with the tile cull on and off, against mjh_ray_device fed the same width x height
world-frame rays (uploaded once) — the only route a caller had before the depth kernel.  Every route is the whole call: the
position-stage launch plus its kernel, event-timed on the engine's stream.  The routes alternate inside every trial, so a drift of the
machine hits all of them; the figures are the median and the range of the trials' means.

Scenes: S24 (rebuilt from the scene's own tables with a static camera above the pen, per-env sizes and poses, settled) and the
106-geom tetrahedron field of tests/ray_mesh_ref.py in mesh mode 1, a static camera above it.

    python tools/depth_bench.py [--nenv 4096] [--width 64] [--height 48] [--reps 200] [--trials 5] [--out FILE]
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

S24_VIEW = ((0.05, -0.1, 2.2), (0.0, 0.0, 0.2), 50.0)
TETRA_VIEW = ((0.3, -1.5, 6.0), (0.0, 0.0, 0.6), 55.0)


def look_at(eye, target):
    """camera frame (columns x right, y up, z backwards): x = f x (0, 0, 1) normalised, y = x x f, z = -f"""
    f = np.asarray(target, float) - np.asarray(eye, float); f /= np.linalg.norm(f)
    x = np.cross(f, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
    return np.stack([x, np.cross(x, f), -f], axis=1)


def mat2quat(R):
    q = np.array([np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2,
                  np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2]),
                  np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0]),
                  np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])])
    return q / np.linalg.norm(q)


def world_rays(view, width, height):
    """the camera's pixel rays in the world frame (fp64), row-major from the top left"""
    eye, target, fovy = view
    t, a = np.tan(np.radians(fovy) / 2), width / height
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    Dc = np.stack([a * t * (2 * (j + 0.5) / width - 1), t * (1 - 2 * (i + 0.5) / height), -np.ones((height, width))], axis=-1).reshape(-1, 3)
    return np.tile(np.asarray(eye, float), (len(Dc), 1)), Dc @ look_at(eye, target).T


def add_camera(lib, b, view):
    from helpers import D
    eye, target, fovy = view
    cid = lib.mjh_builder_add_camera(b, b"cam", 0, D(*eye), D(*mat2quat(look_at(eye, target))), fovy)
    assert cid == 0, lib.mjh_last_error()


def s24_with_camera(lib, extra=None):
    """mjh_scene_s24 has no camera and a compiled model takes none: the same scene built again from its own tables.  extra(lib, b): further
    builder calls before the compile step (tools/light_bench.py adds its lights)"""
    import mujoco_sim_amd as ms
    from helpers import D
    s = ms.scene("s24")
    b = lib.mjh_builder_create()
    lib.mjh_builder_set_option(b, C.byref(s.c.opt))
    lib.mjh_builder_set_capacity(b, s.c.maxcon, s.c.maxefc)
    bp, bq = s.array("body_pos").reshape(-1, 3), s.array("body_quat").reshape(-1, 4)
    gt, gb, gs = s.array("geom_type"), s.array("geom_bodyid"), s.array("geom_size").reshape(-1, 3)
    gp, gq, gf = s.array("geom_pos").reshape(-1, 3), s.array("geom_quat").reshape(-1, 4), s.array("geom_friction").reshape(-1, 3)
    cd, ct, ca = s.array("geom_condim"), s.array("geom_contype"), s.array("geom_conaffinity")
    ids = {0: 0}
    for k in range(1, s.c.nbody):
        ids[k] = lib.mjh_builder_add_body(b, lib.mjh_id2name(s.ptr, 0, k), 0, D(*bp[k]), D(*bq[k]), 0.0)
        lib.mjh_builder_add_joint(b, lib.mjh_id2name(s.ptr, 1, k - 1), ids[k], 0, None, None, None, 0, 0, 0, 0, 0)
    for g in range(s.c.ngeom):
        assert lib.mjh_builder_add_geom(b, lib.mjh_id2name(s.ptr, 2, g), ids[int(gb[g])], int(gt[g]), D(*gs[g]), D(*gp[g]), D(*gq[g]), D(*gf[g]),
                                        int(cd[g]), int(ct[g]), int(ca[g]), -1) >= 0
    add_camera(lib, b, S24_VIEW)
    if extra:
        extra(lib, b)
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    for n in ("geom_type", "geom_bodyid", "geom_size", "geom_pos", "body_mass", "qpos0", "pair_geom1", "pair_geom2"):
        assert np.array_equal(m.array(n), s.array(n)), n      # (the per-env tables of mjh_scene_s24_randomize address this layout)
    return m, s


def tetra_with_camera(lib, extra=None):
    import mujoco_sim_amd as ms
    import ray_mesh_ref as rm
    import ray_ref as rr
    from helpers import D, set_opt
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    v = np.ascontiguousarray(0.4 * rm.tetra_points(), float)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    for k, g in enumerate(rm.tetra_field_spec()):
        if g["type"] == rr.MESH:
            assert lib.mjh_builder_add_mesh_geom(b, b"g%d" % k, 0, mid, D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
        else:
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
    bd = lib.mjh_builder_add_body(b, b"far", 0, D(0, 0, 50.0), None, 0.0)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"fg", bd, rr.SPHERE, D(0.05, 0, 0), None, None, None, -1, 0, 0, -1)
    add_camera(lib, b, TETRA_VIEW)
    if extra:
        extra(lib, b)
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--reps", type=int, default=200, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=5, help="timed windows per route (the routes alternate)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=200, help="S24: steps before the images")
    ap.add_argument("--scenes", nargs="+", default=["s24", "tetra"])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mujoco_sim_amd as ms
    from mujoco_sim_amd import capi

    lib = capi.load()
    dev = torch.device("cuda:0")
    W, H, n = args.width, args.height, args.nenv
    res = dict(nenv=n, width=W, height=H, reps=args.reps, trials=args.trials, device=torch.cuda.get_device_name(0), scenes=[])
    for name in args.scenes:
        if name == "s24":
            m, s = s24_with_camera(lib)
            e = ms.Engine(m, n)
            t = s.s24_randomize(0, n)
            for k in ["geom_size", "geom_rbound", "body_mass", "body_inertia", "body_invweight0", "dof_invweight0"]:
                e.set_env_param(k, t[k])
            e.set_initial_qpos(t["qpos"]); e.reset()
            e.step(args.settle); e.synchronize()
            view = S24_VIEW
        else:
            m = tetra_with_camera(lib)
            e = ms.Engine(m, n)
            e.ray_mesh_mode = 1
            view = TETRA_VIEW
        P, V = world_rays(view, W, H)
        tp = torch.tensor(P, dtype=torch.float32, device=dev); tv = torch.tensor(V, dtype=torch.float32, device=dev)
        out = {r: (torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.int32, device=dev))
               for r in ("depth_cull1", "depth_cull0", "ray_device")}
        routes = {
            "depth_cull1": lambda d, g: e.depth_device(d.data_ptr(), g.data_ptr(), 0, W, H, cull=1),
            "depth_cull0": lambda d, g: e.depth_device(d.data_ptr(), g.data_ptr(), 0, W, H, cull=0),
            "ray_device": lambda d, g: e.ray_device(tp.data_ptr(), tv.data_ptr(), d.data_ptr(), g.data_ptr(), W * H),
        }
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
        d1, g1 = img["depth_cull1"]; d0, g0 = img["depth_cull0"]; dr, gr = img["ray_device"]
        same = g1 == gr
        case = dict(scene=name, ngeom=int(m.c.ngeom), mesh_mode=e.ray_mesh_mode, hit_share=float((g1 >= 0).mean()),
                    geoms_seen=int(len(np.unique(g1[g1 >= 0]))),
                    cull_bitwise_equal=bool(np.array_equal(d1.view(np.uint32), d0.view(np.uint32)) and np.array_equal(g1, g0)),
                    ray_route_same_geom_share=float(same.mean()),
                    ray_route_max_abs_diff_where_same_geom=float(np.abs(d1 - dr)[same & (g1 >= 0)].max(initial=0.0)), routes={})
        for r in routes:
            ts = np.array(times[r])
            case["routes"][r] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                                     pixels_per_s=n * W * H / (float(np.median(ts)) * 1e-3))
        med = {r: case["routes"][r]["ms_median"] for r in routes}
        case["cull1_over_cull0"] = med["depth_cull1"] / med["depth_cull0"]
        case["cull1_over_ray_device"] = med["depth_cull1"] / med["ray_device"]
        res["scenes"].append(case)
        e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
