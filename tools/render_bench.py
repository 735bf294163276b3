"""Time of an RGB-D image per env: mjh_depth_device (depth and geom id) against mjh_render_device (the same depth launch, then the shade
kernel: normals and colour) on the scenes and sizes of tools/depth_bench.py, in one process.  Every route is the whole call: the
position-stage launch plus its kernels, event-timed on the engine's stream.  The routes alternate inside every trial, so a drift of the
machine hits all of them; the figures are the median and the range of the trials' means, and render / depth is the ratio of the medians:
what the second launch and its 8 bytes of re-read per pixel cost.

    python tools/render_bench.py [--nenv 4096] [--width 64] [--height 48] [--reps 200] [--trials 5] [--out FILE]
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
    from depth_bench import s24_with_camera, tetra_with_camera
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
        else:
            m = tetra_with_camera(lib)
            e = ms.Engine(m, n)
            e.ray_mesh_mode = 1
        buf = {r: (torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W), dtype=torch.int32, device=dev))
               for r in ("depth", "render", "render_rgba_only")}
        nrm = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev)
        col = {r: torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev) for r in ("render", "render_rgba_only")}
        routes = {
            "depth": lambda: e.depth_device(buf["depth"][0].data_ptr(), buf["depth"][1].data_ptr(), 0, W, H),
            "render": lambda: e.render_device(buf["render"][0].data_ptr(), buf["render"][1].data_ptr(), nrm.data_ptr(), col["render"].data_ptr(), 0, W, H),
            "render_rgba_only": lambda: e.render_device(buf["render_rgba_only"][0].data_ptr(), buf["render_rgba_only"][1].data_ptr(), None,
                                                        col["render_rgba_only"].data_ptr(), 0, W, H),
        }
        torch.cuda.synchronize()
        for f in routes.values():
            for _ in range(args.warmup):
                f()
        e.synchronize()
        times = {r: [] for r in routes}
        for _ in range(args.trials):
            for r, f in routes.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    f()
                b.record(); b.synchronize()
                times[r].append(a.elapsed_time(b) / args.reps)
        d0, g0 = (x.cpu().numpy() for x in buf["depth"]); d1, g1 = (x.cpu().numpy() for x in buf["render"])
        nn = nrm.cpu().numpy(); hit = g1 >= 0
        case = dict(scene=name, ngeom=int(m.c.ngeom), mesh_mode=e.ray_mesh_mode, hit_share=float(hit.mean()), geoms_seen=int(len(np.unique(g1[hit]))),
                    depth_bitwise_equal=bool(np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(g0, g1)),
                    rgba_bitwise_equal=bool(np.array_equal(col["render"].cpu().numpy(), col["render_rgba_only"].cpu().numpy())),
                    unit_normals_on_hits=bool(np.abs(np.linalg.norm(nn[hit], axis=1) - 1.0).max(initial=0.0) < 1e-5), routes={})
        for r in routes:
            ts = np.array(times[r])
            case["routes"][r] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                                     pixels_per_s=n * W * H / (float(np.median(ts)) * 1e-3))
        med = {r: case["routes"][r]["ms_median"] for r in routes}
        case["render_over_depth"] = med["render"] / med["depth"]
        case["render_rgba_only_over_depth"] = med["render_rgba_only"] / med["depth"]
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
