"""Every dist / geomid / depth / normal / rgba array of a fixed set of small scenes in one .npz: the bit-for-bit A/B of two builds of the library
(MJHIP_LIB selects the build).  The scenes are the smallest that reach each path the ray and depth kernels share, at 4 envs, made
with the builders of the GPU tests: the primitives with a camera and a site on a free body (world-frame rays of 1, 63, 65 and 130;
site-frame rays; per-env rays; bodyexclude, flg_static = 0, a cutoff; per-env geom sizes; an inactive slot), the height field, the
mesh model in mesh modes 0 and 1, the tetrahedron field in mesh mode 1, more than 64 spheres; images of 1x1, 9x8 and 30x20 with the
cull on and off and range on and off.  Mesh surface 1 (the meshes' own triangles) for the mesh model and the tetrahedron field, through
both calls.  For every camera and size mjh_render's normal and rgba images with range on and off, and the models of the render tests
(tests/render_check.py): the height field from the side and from below (its base and walls), the meshes as hulls and as triangles.
The other kernels that trace per tile, with the builders of their GPU tests: mjh_scan (range, geom id, points) on the primitives from the
world frame and from a site on a free ball, in every tile shape, with an elevation table, a cutoff, cull on and off, over more than 64
spheres and through mesh surface 1; mjh_heightscan at 1 x 1, 9 x 5 and 17 x 16 in the three alignments with exclude_tree and the cull
on and off, over a plane, the primitives, the height field, more than 64 spheres and mesh surface 1; mjh_render with lighting 1 for the
models of tests/light_check.py (spot, directional and positional lights), shadows and the light cull on and off, once with texturing 1.

    python tools/ray_depth_dump.py OUT.npz
    python tools/ray_depth_dump.py --compare A.npz B.npz      (exit status 1 and the first array that differs, if any)
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NENV = 4
SIZES = [(1, 1), (9, 8), (30, 20)]


def compare(a, b):
    A, B = np.load(a), np.load(b)
    if sorted(A.files) != sorted(B.files):
        print(f"different sets of arrays: {sorted(set(A.files) ^ set(B.files))}")
        return 1
    for k in sorted(A.files):
        x, y = A[k], B[k]
        if x.dtype != y.dtype or x.shape != y.shape or x.tobytes() != y.tobytes():
            n = int((x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8)).sum()) if x.shape == y.shape and x.dtype == y.dtype else -1
            print(f"{k} differs ({x.dtype} {x.shape} against {y.dtype} {y.shape}, {n} bytes)")
            return 1
    print(f"{len(A.files)} arrays, {sum(A[k].nbytes for k in A.files)} bytes: equal byte for byte")
    return 0


def dump(path):
    import mujoco_sim_amd as ms
    import ray_mesh_ref as rm
    import ray_ref as rr
    import render_check as rc
    import test_gpu_depth as td
    from depth_bench import TETRA_VIEW, tetra_with_camera, world_rays
    from helpers import D, set_opt
    from mujoco_sim_amd import capi

    lib = capi.load()
    out = {}

    def rays(tag, e, P, V, **kw):
        d, g = e.ray(P, V, **kw)
        out[tag + "/dist"], out[tag + "/geomid"] = d, g

    def images(tag, e, cam, sizes=SIZES, **kw):
        for w, h in sizes:
            for cull in (0, 1):
                for rng in (0, 1):
                    d, g = e.depth(cam, w, h, cull=cull, range=rng, **kw)
                    out[f"{tag}/{w}x{h}/cull{cull}/range{rng}/depth"], out[f"{tag}/{w}x{h}/cull{cull}/range{rng}/geomid"] = d, g
            for rng in (0, 1):
                d, g, nrm, col = e.render(cam, w, h, range=rng, **kw)
                for k, a in (("depth", d), ("geomid", g), ("normal", nrm), ("rgba", col)):
                    out[f"{tag}/{w}x{h}/render/range{rng}/{k}"] = a

    def prim_model():
        """the primitives with the two static views, and a free ball that carries a camera and a site"""
        b = lib.mjh_builder_create()
        set_opt(lib, b, timestep=0.002, gravity=[0, 0, 0])
        td.add_spec(lib, b, rr.primitives_spec())
        td.add_camera(lib, b, b"front", 0, td.VIEW_FRONT)
        td.add_camera(lib, b, b"side", 0, td.VIEW_SIDE)
        bd = lib.mjh_builder_add_body(b, b"rig", 0, D(0.0, -3.5, 2.5), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_geom(b, b"rigg", bd, rr.SPHERE, D(td.RIG_RADIUS, 0, 0), None, None, None, -1, -1, -1, -1) >= 0
        assert lib.mjh_builder_add_camera(b, b"eye", bd, D(*td.RIG_CAM_POS), D(*td.RIG_CAM_QUAT), 60.0) == 2
        site = lib.mjh_builder_add_site(b, b"laser", bd, D(0.12, 0.0, 0.02), D(*td.RIG_CAM_QUAT))
        assert site >= 0
        return td.compile_model(lib, b), bd, site

    # ---- the primitives: every option of the two calls
    m, rig, site = prim_model()
    e = ms.Engine(m, NENV)
    rng = np.random.default_rng(23)
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[rig]])
    q = np.tile(m.array("qpos0"), (NENV, 1))
    for i in range(NENV):      # the rig looks at the scene from its own place in every env
        eye = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-4.2, -3.2), rng.uniform(2.0, 3.2)])
        q[i, adr:adr + 3] = eye
        q[i, adr + 3:adr + 7] = td.mat2quat(td.look_at(eye, np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.4, 0.4, size=3)) @ rr.quat2mat(td.RIG_CAM_QUAT).reshape(3, 3).T)
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv)))
    e.forward()
    scene = rr.scene_from_spec(rr.primitives_spec())
    P, V = rr.primitive_rays(scene, 130)
    for nray in (1, 63, 65, 130):
        rays(f"prim/world{nray}", e, P[:nray], V[:nray])
    Ps = rng.uniform(-0.02, 0.02, size=(NENV, 130, 3)); Vs = rng.normal(size=(NENV, 130, 3)) * [1.0, 1.0, 3.0] + [0, 0, -3.0]      # (the camera looks along -z)
    rays("prim/site", e, Ps[0], Vs[0], site=site, bodyexclude=rig)
    rays("prim/site_inside", e, Ps[0, :65], Vs[0, :65], site=site)
    rays("prim/site_per_env", e, Ps, Vs, site=site, bodyexclude=rig)
    rays("prim/world_per_env", e, np.stack([P + 0.01 * i for i in range(NENV)]), np.stack([V] * NENV))
    rays("prim/sub_range", e, P, V, env0=1, n=2)
    body = m.array("geom_bodyid")
    bx = int(body[np.nonzero(body > 0)[0][0]])
    rays("prim/bodyexclude", e, P, V, bodyexclude=bx)
    rays("prim/flg_static0", e, P, V, flg_static=0)
    rays("prim/cutoff", e, P, V, cutoff=2.0)
    rays("prim/all_options", e, P, V, bodyexclude=bx, flg_static=0, cutoff=2.5)
    images("prim/front", e, "front")
    images("prim/side", e, "side", sizes=[(9, 8)])
    images("prim/eye", e, "eye", bodyexclude=rig)
    images("prim/eye_inside", e, "eye", sizes=[(9, 8)])
    images("prim/front_options", e, "front", sizes=[(30, 20)], bodyexclude=bx, flg_static=0, cutoff=5.0, env0=1, n=3)
    # per-env geom sizes, then an inactive slot
    small = (0.8 * m.array("geom_size")).astype(np.float32).astype(float)
    e.set_env_param("geom_size", small[None, :], env0=1)
    rays("sizes/world", e, P, V)
    images("sizes/front", e, "front", sizes=[(30, 20)])
    e.set_slot_active(bx, 0, env0=2, n=1)
    rays("slot/world", e, P, V)
    images("slot/front", e, "front", sizes=[(30, 20)])
    e.close()

    # ---- the height field
    b = lib.mjh_builder_create()
    el = (C.c_double * rr.HF_ELEV.size)(*rr.HF_ELEV.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", rr.HF_NROW, rr.HF_NCOL, D(*rr.HF_SIZE), el)
    assert h >= 0 and lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*rr.HF_POS), D(*rr.HF_QUAT), None, -1, -1, -1) >= 0
    td.far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    td.add_camera(lib, b, b"cam", 0, td.VIEW_HFIELD)
    e = ms.Engine(td.compile_model(lib, b), NENV)
    rays("hfield/world", e, *rr.hfield_rays(rr.hfield_scene()))
    images("hfield/cam", e, "cam", sizes=[(9, 8), (30, 20)])
    e.close()

    # ---- mesh geoms: the mesh model in both modes, the tetrahedron field in mode 1
    b = lib.mjh_builder_create()
    v = np.ascontiguousarray(rm.box_points(), float)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    assert mid >= 0
    lib.mjh_builder_add_geom(b, b"floor", 0, rr.PLANE, D(0, 0, 0.05), None, None, None, -1, -1, -1, -1)
    for k in range(2):
        bd = lib.mjh_builder_add_body(b, b"m%d" % k, 0, D(0.9 * k, 0, 1.0), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, bd, mid, None, None, None, -1, -1, -1, -1) >= 0
    lib.mjh_builder_add_geom(b, b"ball", 0, rr.SPHERE, D(0.2, 0, 0), D(0, 0, 0.4), None, None, -1, -1, -1, -1)
    td.add_camera(lib, b, b"cam", 0, td.VIEW_MESH)
    e = ms.Engine(td.compile_model(lib, b), NENV)
    Pm, Vm = world_rays(td.VIEW_MESH, 13, 10)
    for mode in (0, 1):
        e.ray_mesh_mode = mode
        rays(f"mesh/mode{mode}/world", e, Pm, Vm)
        images(f"mesh/mode{mode}/cam", e, "cam", sizes=[(9, 8), (30, 20)])
    e.ray_mesh_surface = 1
    rays("mesh/surface1/world", e, Pm, Vm)
    images("mesh/surface1/cam", e, "cam", sizes=[(9, 8), (30, 20)])
    e.close()
    e = ms.Engine(tetra_with_camera(lib), NENV)
    e.ray_mesh_mode = 1
    for surface in (0, 1):
        e.ray_mesh_surface = surface
        tag = "tetra" if surface == 0 else "tetra/surface1"
        rays(tag + "/world", e, *world_rays(TETRA_VIEW, 13, 10))
        images(tag + "/cam", e, 0)
    e.close()

    # ---- the render tests' models: the height field's top, walls and base, the non-convex meshes as hulls and as triangles
    e = ms.Engine(rc.hfield_model(lib), NENV)
    images("render_hfield/cam", e, "cam", sizes=[(9, 8), (30, 20)])
    images("render_hfield/under", e, "under", sizes=[(9, 8), (30, 20)])
    e.close()
    mm, _ = rc.meshes_model(lib)
    e = ms.Engine(mm, NENV)
    e.ray_mesh_mode = 1
    Pr, Vr = world_rays(rc.VIEW_MESHES, 13, 10)
    for surface in (0, 1):
        e.ray_mesh_surface = surface
        rays(f"render_meshes/surface{surface}/world", e, Pr, Vr)
        images(f"render_meshes/surface{surface}/cam", e, "cam", sizes=[(9, 8), (24, 16)])
    e.close()

    # ---- more geoms than one staging pass holds
    spec = rr.many_spheres_spec()
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    td.add_spec(lib, b, spec)
    td.far_body(lib, b)
    td.add_camera(lib, b, b"above", 0, td.VIEW_SPHERES)
    e = ms.Engine(td.compile_model(lib, b), NENV)
    rays("spheres/world", e, *rr.many_spheres_rays(rr.scene_from_spec(spec)))
    images("spheres/above", e, "above")
    e.close()

    # ---- the kernels that trace per tile besides depth: lidar scans, height scans, lit (and textured) renders
    import heightscan_ref as hr
    import light_check as lc
    import scan_ref as sr
    import test_gpu_heightscan as th
    import test_gpu_scan as ts
    import texture_check as tc

    def scans(tag, e, site, patterns, **kw):
        for name, pattern in patterns:
            for cull in (0, 1):
                r, g, pts = e.scan(site, **sr.scan_kwargs(pattern), cull=cull, points=True, **kw)
                for k, a in (("range", r), ("geomid", g), ("points", pts)):
                    out[f"{tag}/{name}/cull{cull}/{k}"] = a

    def hscans(tag, e, site, grids, aligns=hr.ALIGNS, **kw):
        for w, h in grids:
            for align in aligns:
                for cull in (0, 1):
                    r, g, pts = e.height_scan(site, **hr.kwargs((w, h, (0.11, 0.09), (0.05, -0.03), 0.5)), align=align, cull=cull, points=True, **kw)
                    for k, a in (("range", r), ("geomid", g), ("points", pts)):
                        out[f"{tag}/{w}x{h}/{align}/cull{cull}/{k}"] = a

    def lit(tag, e, cam, sizes=SIZES):
        for w, h in sizes:
            for shadows in (0, 1):
                for cull in (0, 1):
                    e.light_options = dict(shadows=shadows, cull=cull)
                    for k, a in zip(("depth", "geomid", "normal", "rgba"), e.render(cam, w, h)):
                        out[f"{tag}/{w}x{h}/shadows{shadows}/cull{cull}/{k}"] = a

    # every tile shape scan_tile_shape returns (1 x 64, 2 x 32, 4 x 16, 8 x 8), partial tiles in both directions, an elevation table
    PATTERNS = [("360x1", (360, 1, -np.pi, 2 * np.pi / 360, (0.0, 0.0))), ("40x2", (40, 2, -1.0, 0.05, (-0.3, 0.2))), ("20x3", (20, 3, 0.4, 0.06, (-0.5, 0.2))),
                ("33x5", (33, 5, -1.9, 0.11, (-0.6, 0.2))), ("70x16", (70, 16, -np.pi, 2 * np.pi / 70, (-0.9, 0.1))), ("table 9x70", sr.PATTERNS["table 9x70"])]
    m = ts.prim_model(lib, rig=True)
    e = ms.Engine(m, NENV)
    e.set_state(qpos=ts.rig_qpos(m), qvel=np.zeros((NENV, m.nv)))
    e.forward()
    rig = m.name2id(0, "rig")
    scans("scan/world", e, None, PATTERNS)
    scans("scan/site", e, "head", PATTERNS, bodyexclude=rig)
    scans("scan/site_cutoff", e, "head", PATTERNS[3:4], bodyexclude=rig, cutoff=1.5)
    e.close()
    e = ms.Engine(ts.spheres_model(lib), NENV)
    scans("scan/spheres", e, "lidar", [("128x8", ts.SPHERES_PATTERN)])
    e.close()
    e = ms.Engine(ts.tri_model(lib), NENV)
    e.ray_mesh_mode = 1; e.ray_mesh_surface = 1
    scans("scan/surface1", e, "scanner", [("96x8", ts.TRI_PATTERN)])
    hscans("hscan/surface1", e, "scanner", [(17, 16)], aligns=("yaw",))
    e.close()

    GRIDS = [(1, 1), (9, 5), (17, 16)]
    m = th.tree_model(lib)      # a floor (a plane), a base with an arm, another body: exclude_tree hides the first two
    e = ms.Engine(m, NENV)
    q = np.tile(m.array("qpos0"), (NENV, 1))
    q[:, int(m.array("jnt_qposadr")[m.name2id(1, "elbow")])] = [0.0, 0.3, -0.4, 0.7]
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv))); e.forward()
    base = m.name2id(0, "base")
    for tree in (0, 1):
        hscans(f"hscan/plane/tree{tree}", e, "head", GRIDS, bodyexclude=base, exclude_tree=tree)
    e.close()
    m = th.prim_model(lib, rig=True)
    e = ms.Engine(m, NENV)
    e.set_state(qpos=th.rig_qpos(m), qvel=np.zeros((NENV, m.nv))); e.forward()
    for tree in (0, 1):
        hscans(f"hscan/prim/tree{tree}", e, "head", GRIDS, bodyexclude=m.name2id(0, "rig"), exclude_tree=tree)
    e.close()
    e = ms.Engine(th.hfield_model(lib, (rr.HF_NROW, rr.HF_NCOL, np.array(rr.HF_SIZE), rr.HF_ELEV), rr.HF_POS, rr.HF_QUAT, th.HFIELD_SENSOR), NENV)
    hscans("hscan/hfield", e, "scanner", GRIDS)
    e.close()
    e = ms.Engine(th.spheres_model(lib), NENV)
    hscans("hscan/spheres", e, "scanner", GRIDS)
    e.close()

    m = lc.prim_model(lib, lights=(lc.SPOT, lc.SUN, lc.LOW_SPOT))      # a spot, a directional and a positional light inside the scene
    e = ms.Engine(m, NENV)
    e.render_lighting = 1
    lit("light/prim/front", e, "front")
    lit("light/prim/side", e, "side", sizes=[(9, 8)])
    e.close()
    e = ms.Engine(lc.spheres_model(lib), NENV)
    e.render_lighting = 1
    lit("light/spheres", e, "above")
    e.close()
    e = ms.Engine(lc.hfield_model(lib), NENV)
    e.render_lighting = 1
    lit("light/hfield", e, "cam", sizes=[(9, 8), (30, 20)])
    e.close()
    e = ms.Engine(lc.meshes_model(lib)[0], NENV)
    e.render_lighting = 1; e.ray_mesh_mode = 1; e.ray_mesh_surface = 1
    lit("light/surface1", e, "cam", sizes=[(9, 8), (24, 16)])
    e.close()
    e = ms.Engine(tc.prim_model(lib, lights=(lc.SPOT, lc.SUN)), NENV)
    e.render_lighting = 1; e.render_texturing = 1
    lit("light/textured", e, "front")
    e.close()

    hits = {k: float((a >= 0).mean()) for k, a in out.items() if k.endswith("geomid")}
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    np.savez(path, **out)
    print(f"{path}: {len(out)} arrays, {sum(a.nbytes for a in out.values())} bytes from {capi.LIB_PATH}; smallest hit share {min(hits.values()):.3f} ({min(hits, key=hits.get)})")
    return 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    sys.exit(dump(sys.argv[1]))
