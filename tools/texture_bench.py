"""Time of a textured colour image per env: mjh_render_device at lighting 0 and lighting 1 (two lights, shadows on), each with
texturing 0 and texturing 1 (the texture kernel between the depth and shade launches), on the primitives scene of the tests with the
512 x 512 checker on its floor and 8 x 8 textures on four small geoms, in one process.  Every route is the whole call: the
position-stage launch plus its kernels, event-timed on the engine's stream.  The routes alternate inside every trial, so a drift of the
machine hits all of them; the figures are the median and the range of the trials' means, and texturing 1 is reported against
texturing 0 of the same lighting mode of the same run.

    python tools/texture_bench.py [--nenv 4096] [--width 64] [--height 48] [--reps 100] [--trials 5] [--out profiles/texture_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nenv", type=int, default=4096)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--height", type=int, default=48)
    ap.add_argument("--reps", type=int, default=100, help="calls per timed window")
    ap.add_argument("--trials", type=int, default=5, help="timed windows per route (the routes alternate)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--camera", default="front")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import light_check as lc
    import mujoco_sim_amd as ms
    import texture_check as tc
    from mujoco_sim_amd import capi

    lib = capi.load()
    dev = torch.device("cuda:0")
    W, H, n = args.width, args.height, args.nenv
    m = tc.prim_model(lib, coloured=True, lights=(lc.SPOT, lc.SUN))
    assert m.ntex == 4 and m.nlight == 2
    e = ms.Engine(m, n)
    depth = torch.empty((n, H, W), dtype=torch.float32, device=dev); gid = torch.empty((n, H, W), dtype=torch.int32, device=dev)
    nrm = torch.empty((n, H, W, 3), dtype=torch.float32, device=dev); col = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)

    def call():
        e.render_device(depth.data_ptr(), gid.data_ptr(), nrm.data_ptr(), col.data_ptr(), args.camera, W, H)

    def route(lighting, texturing):
        def f():
            e.render_lighting = lighting
            e.render_texturing = texturing
        return f
    routes = {f"light{l}_tex{t}": route(l, t) for l in (0, 1) for t in (0, 1)}
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
    textured = np.isin(g, [k for k, t in enumerate(m.array("geom_texid")) if t >= 0])
    res = dict(nenv=n, width=W, height=H, reps=args.reps, trials=args.trials, device=torch.cuda.get_device_name(0), scene="primitives, textured floor",
               camera=args.camera, ngeom=int(m.c.ngeom), ntex=int(m.ntex), ntexdata=int(m.ntexdata), hit_share=float((g >= 0).mean()),
               textured_share=float(textured.mean()), routes={},
               untextured_pixels_equal={f"light{l}": bool(np.array_equal(images[f"light{l}_tex0"][~textured], images[f"light{l}_tex1"][~textured])) for l in (0, 1)},
               changed_share={f"light{l}": float((images[f"light{l}_tex0"] != images[f"light{l}_tex1"]).any(axis=-1).mean()) for l in (0, 1)})
    for r in routes:
        ts = np.array(times[r])
        res["routes"][r] = dict(ms_median=float(np.median(ts)), ms_min=float(ts.min()), ms_max=float(ts.max()), pixels_per_s=n * W * H / (float(np.median(ts)) * 1e-3))
    for l in (0, 1):
        res["routes"][f"light{l}_tex1"]["over_tex0"] = res["routes"][f"light{l}_tex1"]["ms_median"] / res["routes"][f"light{l}_tex0"]["ms_median"]
    e.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
