"""What the mesh's own triangles cost a ray: the PR2 world model (the world file's floor + PR2 with its mesh assets) in mesh mode 1 with
mesh surface 0 (convex hulls) and 1 (the assets' triangles through their BVHs) — the fan of tests/ray_mesh_ref.pr2_fan() through
mjh_ray_device, and a 64 x 64 depth image from a camera at the fan's origin through mjh_depth_device.  Event-timed on the engine's
stream; the two surfaces alternate, `trials` timed windows of `reps` calls each after a warm-up of every shape, and the figures are the
medians with the windows' min and max.  The model is compiled by the MJCF loader from the bundled model files (tests/refmodels.py) with
a camera added to the world.

    python tools/ray_tri_bench.py [--nenv 1024] [--reps 50] [--trials 5] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

EYE, TARGET, FOVY = (2.0, 0.0, 1.0), (0.0, 0.0, 0.8), 40.0


def look_at_quat(eye, target):
    """quaternion of the camera frame (x right, y up, z backwards) looking from eye at target"""
    f = np.asarray(target, float) - np.asarray(eye, float); f /= np.linalg.norm(f)
    x = np.cross(f, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
    R = np.stack([x, np.cross(x, f), -f], axis=1)
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    q = np.array([w, np.copysign(np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2, R[2, 1] - R[1, 2]),
                  np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2, R[0, 2] - R[2, 0]),
                  np.copysign(np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2, R[1, 0] - R[0, 1])])
    return q / np.linalg.norm(q)


def pr2_with_camera(lib):
    """the PR2 world model with a fixed camera: the world and robot files, plus a third file that holds the camera"""
    import tempfile

    import mujoco_sim_amd as ms
    import ray_mesh_ref as rm
    from refmodels import model_dir
    ref = os.path.join(model_dir(), "test")
    q = look_at_quat(EYE, TARGET)
    with tempfile.TemporaryDirectory() as tmp:
        cam = os.path.join(tmp, "camera.xml")
        with open(cam, "w") as f:
            f.write('<mujoco><worldbody><camera name="scan" pos="%g %g %g" quat="%.17g %.17g %.17g %.17g" fovy="%g"/></worldbody></mujoco>\n' % (*EYE, *q, FOVY))
        lib.mjh_load_set_bounds(1e-6, 1e-6); lib.mjh_load_set_mesh_mode(1)
        try:
            m = ms.load_mjcf(paths=[os.path.join(ref, "..", "world", "empty.xml"), os.path.join(ref, rm.ROBOT_FILES["pr2"]), cam])
        finally:
            lib.mjh_load_set_bounds(0.0, 0.0)
    z = np.load(os.path.join(ROOT, "tests", "golden", "robot_pr2_world_mesh.npz"))
    m.c.maxcon = int(z["int__maxcon"]); m.c.maxefc = int(z["int__maxefc"])
    assert m.ncam == 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=50, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=5, help="timed windows per case (the surfaces alternate)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--size", type=int, default=64, help="depth image width = height")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mujoco_sim_amd as ms
    import ray_mesh_ref as rm
    from mujoco_sim_amd import capi

    assert torch.cuda.is_available(), "this is a measurement on the GPU: there is no other route"
    lib = capi.load()
    m = pr2_with_camera(lib)
    types = m.array("geom_type")
    n, S = args.nenv, args.size
    e = ms.Engine(m, n)
    e.ray_mesh_mode = 1
    dev = torch.device("cuda:0")
    P, V = rm.pr2_fan()
    nray = len(P)
    tp = torch.tensor(P, dtype=torch.float32, device=dev); tv = torch.tensor(V, dtype=torch.float32, device=dev)
    rd = torch.empty((n, nray), dtype=torch.float32, device=dev); rg = torch.empty((n, nray), dtype=torch.int32, device=dev)
    dd = torch.empty((n, S, S), dtype=torch.float32, device=dev); dg = torch.empty((n, S, S), dtype=torch.int32, device=dev)
    routes = {
        "ray_fan": (lambda: e.ray_device(tp.data_ptr(), tv.data_ptr(), rd.data_ptr(), rg.data_ptr(), nray), n * nray, rg),
        "depth": (lambda: e.depth_device(dd.data_ptr(), dg.data_ptr(), 0, S, S), n * S * S, dg),
    }
    torch.cuda.synchronize()
    for surface in (0, 1):      # warm-up of every shape with both tables (the first call with surface 1 builds and uploads the BVHs)
        e.ray_mesh_surface = surface
        for f, _, _ in routes.values():
            for _ in range(args.warmup):
                f()
    e.synchronize()
    times = {(r, s): [] for r in routes for s in (0, 1)}
    seen = {}
    for _ in range(args.trials):
        for r, (f, _, g) in routes.items():
            for surface in (0, 1):
                e.ray_mesh_surface = surface
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    f()
                b.record(); b.synchronize()
                times[(r, surface)].append(a.elapsed_time(b) / args.reps)
                seen[(r, surface)] = g[0].cpu().numpy().ravel()
    res = dict(scene="pr2_world_mesh", nenv=n, reps=args.reps, trials=args.trials, ngeom=int(m.ngeom), mesh_geoms=int((types == 7).sum()),
               mesh_planes=int(m.c.nmeshplane), mesh_triangles=int(m.nmeshtri), nray=nray, depth_size=S, device=torch.cuda.get_device_name(0), cases=[])
    for (r, surface), ts in times.items():
        ts = np.array(ts); g = seen[(r, surface)]; hit = g >= 0
        res["cases"].append(dict(route=r, mesh_surface=surface, ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                                 per_s=routes[r][1] / (float(np.median(ts)) * 1e-3), hit_share=float(hit.mean()),
                                 mesh_hit_share=float((types[g[hit]] == 7).mean()) if hit.any() else 0.0))
    for r in routes:
        c = {c["mesh_surface"]: c for c in res["cases"] if c["route"] == r}
        res[f"{r}_triangles_over_hull"] = c[1]["ms_median"] / c[0]["ms_median"]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    e.close()


if __name__ == "__main__":
    main()
