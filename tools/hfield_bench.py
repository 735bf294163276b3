"""Height-field terrain scene at 4096 envs: env-steps/s of mjh_step on terrain and on the same scene with a plane floor.

  python tools/hfield_bench.py [--envs 4096] [--steps 200] [--warmup 50] [--floor hfield|plane|both]

Four free bodies (two spheres, a box, a cylinder) per env dropped over a 32 x 32 terrain (or a plane at the terrain's mean
height); contact capacity 64, so the scene takes the window chain like S24.  One JSON line per floor.  For the assemble
launch's kernel time, run one floor under `rocprofv3 --kernel-trace --stats -- python tools/hfield_bench.py --floor hfield`
(and again with --floor plane) and read mjh_step_kernel's row of the stats."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mujoco_sim_amd as ms  # noqa: E402
from mujoco_sim_amd import capi  # noqa: E402


def D(*a):
    return (C.c_double * len(a))(*a)


def model(lib, floor, nrow=32, ncol=32, size=(1.5, 1.5, 0.15, 0.3), seed=11):
    rng = np.random.default_rng(seed)
    x, y = np.meshgrid(np.linspace(0, 1, ncol), np.linspace(0, 1, nrow))
    elev = (np.sin(6 * x + 1.0) * np.cos(5 * y + 2.0) + 0.3 * rng.normal(size=(nrow, ncol))).ravel()
    b = lib.mjh_builder_create()
    o = capi.Option(); lib.mjh_builder_get_option(b, C.byref(o)); o.timestep = 0.002; lib.mjh_builder_set_option(b, C.byref(o))
    lib.mjh_builder_set_capacity(b, 64, 0)
    if floor == "hfield":
        h = lib.mjh_builder_add_hfield(b, b"terrain", nrow, ncol, D(*size), (C.c_double * len(elev))(*elev))
        lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, None, None, None, -1, -1, -1)
    else:
        lib.mjh_builder_add_geom(b, b"ground", 0, 0, D(5, 5, 0.1), D(0, 0, 0.5 * size[2]), None, None, -1, -1, -1, -1)
    shapes = [(2, (0.07, 0, 0)), (6, (0.08, 0.06, 0.05)), (2, (0.05, 0, 0)), (5, (0.06, 0.05, 0))]
    for k, (t, s) in enumerate(shapes):
        bd = lib.mjh_builder_add_body(b, b"b%d" % k, 0, D(0.3 * k - 0.45, 0, 0.5), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        lib.mjh_builder_add_geom(b, None, bd, t, D(*s), None, None, None, -1, -1, -1, -1)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    q = np.tile(m.array("qpos0"), (1, 1))
    return m, q, rng


def run(floor, nenv, steps, warmup):
    lib = capi.load()
    m, q0, rng = model(lib, floor)
    q = np.tile(q0, (nenv, 1))
    for i in range(nenv):
        for k in range(4):
            q[i, 7 * k:7 * k + 3] = (*rng.uniform(-1.0, 1.0, size=2), 0.35 + 0.12 * k)
    e = ms.Engine(m, nenv)
    e.set_initial_qpos(q); e.reset()
    e.step(warmup); e.synchronize()
    t0 = time.perf_counter(); e.step(steps); e.synchronize(); dt = time.perf_counter() - t0
    st = e.get_stats()
    e.close()
    return dict(floor=floor, envs=nenv, steps=steps, env_steps_per_s=nenv * steps / dt, ncon_mean=float(st[:, 0].mean()),
                capacity_flags=int((st[:, 3] & 1).sum()))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--floor", choices=["hfield", "plane", "both"], default="both")
    a = ap.parse_args()
    for f in (["hfield", "plane"] if a.floor == "both" else [a.floor]):
        print(json.dumps(run(f, a.envs, a.steps, a.warmup)), flush=True)
