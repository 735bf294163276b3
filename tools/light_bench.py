"""Time of a lit colour image per env: mjh_render_device in lighting mode 0 (the depth launch and the shade kernel) against mode 1 (the
depth launch, the shade kernel writing the normal only, then the light kernel) with 1, 2 and 8 active lights, with shadows on and
off and the occluder cull on and off, on the scenes and sizes of tools/render_bench.py, in one process.  Every route is the whole call:
the position-stage launch plus its kernels, event-timed on the engine's stream.  The routes alternate inside every trial, so a drift of
the machine hits all of them; the figures are the median and the range of the trials' means, and every route is reported against mode 0
of the same run.

The model carries eight lights over the scene (even ids positional spots, odd ids directional); a route switches the first k on with
mjh_set_light_active.

    python tools/light_bench.py [--nenv 4096] [--width 64] [--height 48] [--reps 100] [--trials 5] [--out profiles/light_bench.json]
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


def add_lights(lib, b):
    from helpers import D
    rng = np.random.default_rng(12)
    for k in range(8):
        pos = (float(rng.uniform(-1.0, 1.0)), float(rng.uniform(-1.0, 1.0)), 3.0 + 0.25 * k)
        d = (float(rng.uniform(-0.5, 0.5)), float(rng.uniform(-0.5, 0.5)), -1.0)
        assert lib.mjh_builder_add_light(b, b"l%d" % k, 0, D(*pos), D(*d), k % 2, 1, D(0.3, 0.3, 0.3), D(0.02, 0.02, 0.02), 60.0, 2.0) == k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window")
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
            m, s = s24_with_camera(lib, add_lights)
            e = ms.Engine(m, n)
            t = s.s24_randomize(0, n)
            for k in ["geom_size", "geom_rbound", "body_mass", "body_inertia", "body_invweight0", "dof_invweight0"]:
                e.set_env_param(k, t[k])
            e.set_initial_qpos(t["qpos"]); e.reset()
            e.step(args.settle); e.synchronize()
        else:
            m = tetra_with_camera(lib, add_lights)
            e = ms.Engine(m, n)
            e.ray_mesh_mode = 1
        assert m.nlight == 8
        depth = torch.empty((n, H, W), dtype=torch.float32, device=dev); gid = torch.empty((n, H, W), dtype=torch.int32, device=dev)
        nrm = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev); col = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)

        def call():
            e.render_device(depth.data_ptr(), gid.data_ptr(), nrm.data_ptr(), col.data_ptr(), 0, W, H)

        def route(mode, nl=0, shadows=1, cull=1):
            def f():
                e.render_lighting = mode
                for k in range(8):
                    e.set_light_active(k, k < nl)
                e.light_options = dict(shadows=shadows, cull=cull)
            return f
        routes = {"mode0": route(0)}
        for nl in (1, 2, 8):
            routes[f"lights{nl}"] = route(1, nl)
            routes[f"lights{nl}_nocull"] = route(1, nl, cull=0)
            routes[f"lights{nl}_noshadow"] = route(1, nl, shadows=0)
        images = {}
        torch.cuda.synchronize()
        for r, setup in routes.items():
            setup()
            for _ in range(args.warmup):
                call()
            e.synchronize()
            images[r] = col.cpu().numpy().copy()
        times = {r: [] for r in routes}
        for _ in range(args.trials):
            for r, setup in routes.items():
                setup()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(args.reps):
                    call()
                b.record(); b.synchronize()
                times[r].append(a.elapsed_time(b) / args.reps)
        g = gid.cpu().numpy()
        case = dict(scene=name, ngeom=int(m.c.ngeom), mesh_mode=e.ray_mesh_mode, hit_share=float((g >= 0).mean()), routes={},
                    cull_bitwise_equal=bool(all(np.array_equal(images[f"lights{k}"], images[f"lights{k}_nocull"]) for k in (1, 2, 8))),
                    shadowed_share={f"lights{k}": float((images[f"lights{k}"] != images[f"lights{k}_noshadow"]).any(axis=-1).mean()) for k in (1, 2, 8)})
        for r in routes:
            ts = np.array(times[r])
            case["routes"][r] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()),
                                     pixels_per_s=n * W * H / (float(np.median(ts)) * 1e-3))
        base = case["routes"]["mode0"]["ms_median"]
        for r in routes:
            case["routes"][r]["over_mode0"] = case["routes"][r]["ms_median"] / base
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
