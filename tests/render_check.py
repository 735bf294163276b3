"""What tests/test_render_host.py (the shade kernel's code on the CPU) and tests/test_gpu_render.py (mjh_render on the device) share:
the models and views, the fp64 rays of a camera, the scene of a model for the references, and the comparison of ONE env's image —
depth, geom id, normal, colour — with tests/render_ref.py.

The comparison.  A pixel is KEPT where the reference is robust in the sense of ray_check (same geom and distance within 1e-3 at the
four 1e-4 shifts of the ray) AND feature-robust (at those shifts the reference names the same feature of the geom, or a normal within
1e-9 of the centre ray's).  The share of pixels left out is capped at ray_check.CAP = 0.02, and the cap is asserted.  On every kept
pixel the geom id agrees; on a kept hit max_c |n - n_ref| <= TOL_N and every colour channel is within 1 + ceil(255 diffuse sqrt(3) TOL_N)
levels (one rounding step plus the normal's error through the shade).  Everywhere: a miss is normal (0, 0, 0) and the background colour
exactly; a hit has a unit normal with n . v <= 0 and alpha 255.

N_HOST is the worst max_c |n_host - n_ref| over the kept pixels of every image of tests/test_render_host.py's IMAGES
(test_n_host_over_the_gpu_scenes: the GPU tests' models, views and image sizes and the 64 x 48 views, rays rounded to float32, cast
through the host build of the kernels' code).  Measured there: 6.475e-6, set by the primitives scene's side view at 30 x 20 (a curved
primitive near grazing); front / side at 64 x 48 give 5.9e-6 / 6.1e-6, the 70 spheres 5.2e-6, the camera inside its ball 1.2e-7, the
height field from above, the hulls and the triangles 1.0e-7 .. 1.2e-7, the height field's base and walls from below 0 (a facet's normal does not depend on the hit point).  N_HOST = 6.5e-6 and
TOL_N = 4 N_HOST = 2.6e-5: the device build differs from the host's in FMA contraction and in its division and square-root sequences
by a few ulps of the hit distance, which a pixel near grazing amplifies.

Excluded shares measured on the CPU (the same test): primitives front 30 x 20 0, 8 x 8 0, 9 x 8 0, 1 x 1 0, 64 x 48 0.0007; side 30 x 20
0.0017, 8 x 8 0.0156 (one pixel of 64), 9 x 8 0, 1 x 1 0, 64 x 48 0.0013; camera inside its ball 0; 70 spheres 16 x 16 0; height field
30 x 20 from above 0.0017, from below (base and two walls) 0.0083; meshes 24 x 16, hulls 0, triangles 0."""
import ctypes as C
import math

import numpy as np

import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr
import ray_tri_ref as rt
import render_ref as rf
from helpers import D, set_opt
from ray_check import CAP, TOL

N_HOST = 6.5e-6
TOL_N = 4 * N_HOST
NENV = 4

# (eye, target, fovy): the static views of tests/test_gpu_depth.py and tests/test_gpu_ray_tri.py
VIEW_FRONT = ((0.2, -4.5, 3.0), (0.0, 0.0, 0.8), 60.0)
VIEW_SIDE = ((3.5, 2.5, 2.2), (0.0, 0.0, 0.8), 45.0)
VIEW_SPHERES = ((0.3, -1.5, 5.5), (0.0, 0.0, 0.6), 55.0)
VIEW_HFIELD = ((0.4, -2.2, 1.6), (0.3, -0.2, 0.3), 50.0)
VIEW_HFIELD_UNDER = ((0.9, -1.5, -1.3), (0.3, -0.2, 0.1), 50.0)      # from below: the base and two walls
MESH_HEIGHT = 1.0
VIEW_MESHES = ((0.0, -0.3, 3.0), (0.0, 0.0, MESH_HEIGHT), 45.0)
TORUS_QUAT = (math.cos(math.radians(12.5)), math.sin(math.radians(12.5)), 0.0, 0.0)      # 25 degrees about x


# ------------------------------------------------------------------ cameras and their rays in fp64
def look_at(eye, target):
    """camera frame (columns x right, y up, z backwards) looking from eye at target: x = f x (0, 0, 1) normalised, y = x x f, z = -f"""
    f = np.asarray(target, float) - np.asarray(eye, float); f /= np.linalg.norm(f)
    x = np.cross(f, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
    y = np.cross(x, f)
    return np.stack([x, y, -f], axis=1)


def mat2quat(R):
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    q = np.array([w, np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1])])
    return q / np.linalg.norm(q)


def pixel_dirs(width, height, fovy):
    """[height * width, 3] camera-frame directions through the pixel centres, row-major from the top left; d.z = -1"""
    t, a = np.tan(np.radians(fovy) / 2), width / height
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([a * t * (2 * (j + 0.5) / width - 1), t * (1 - 2 * (i + 0.5) / height), -np.ones((height, width))], axis=-1).reshape(-1, 3)


def _camera_rays(m, cam, xpos, xquat, width, height):
    b = int(m.array("cam_bodyid")[cam])
    Rb = rr.quat2mat(xquat[b]).reshape(3, 3)
    pos = xpos[b] + Rb @ m.array("cam_pos").reshape(-1, 3)[cam]
    R = Rb @ rr.quat2mat(m.array("cam_quat").reshape(-1, 4)[cam]).reshape(3, 3)
    Dc = pixel_dirs(width, height, float(m.array("cam_fovy")[cam]))
    return np.tile(pos, (len(Dc), 1)), Dc @ R.T


def camera_rays(e, m, cam, env, width, height):
    """world-frame rays of camera `cam` in env `env` from the device's own body pose"""
    xp, xq = e.get_body_state(env, 1)
    return _camera_rays(m, cam, xp[0], xq[0], width, height)


def model_camera_rays(m, cam, width, height):
    """... from the model's own body poses at qpos0 (bodies that hang on the world)"""
    return _camera_rays(m, cam, m.array("body_pos").reshape(-1, 3), m.array("body_quat").reshape(-1, 4), width, height)


# ------------------------------------------------------------------ scenes for the references
def _with_meshes(sc, m, surface):
    """surface None: mesh geoms invisible (mesh mode 0); 0: their hulls (scipy, of the kept vertices; a mesh without hull planes stays
    invisible); 1: their own triangles (a mesh without triangles keeps its hull)"""
    types, did = m.array("geom_type"), m.array("geom_dataid")
    mesh_geoms = np.nonzero(types == rr.MESH)[0]
    if not len(mesh_geoms):
        return sc
    sc["visible"] = sc["visible"].copy()
    if surface is None:
        sc["visible"][mesh_geoms] = False
        return sc
    pnum, tnum = m.array("mesh_planenum"), m.array("mesh_trinum")
    verts, tris = rm.model_mesh_verts(m), rt.model_mesh_tris(m)
    cache = {}
    sc["mesh"] = {}
    for g in mesh_geoms:
        i = int(did[g])
        if i not in cache:
            cache[i] = tris[i] if (surface == 1 and tnum[i] > 0) else (rm.hull_triangles(verts[i]) if pnum[i] > 0 else None)
        if cache[i] is None:
            sc["visible"][g] = False
        else:
            sc["mesh"][int(g)] = cache[i]
    return sc


def model_hfields(m):
    import hfield_ref
    types, did = m.array("geom_type"), m.array("geom_dataid")
    return {int(g): hfield_ref.hfield_of(m, int(g)) for g in np.nonzero(types == rr.HFIELD)[0] if did[g] >= 0}


def model_scene(m, surface=None):
    """the scene of the model at qpos0 from its own arrays (bodies that hang on the world): what an engine shows before a step"""
    bp, bq = m.array("body_pos").reshape(-1, 3), m.array("body_quat").reshape(-1, 4)
    gb, gp, gq = m.array("geom_bodyid"), m.array("geom_pos").reshape(-1, 3), m.array("geom_quat").reshape(-1, 4)
    assert (m.array("body_parentid")[gb] == 0).all()
    pos, mat = [], []
    for g in range(m.ngeom):
        Rb = rr.quat2mat(bq[gb[g]]).reshape(3, 3)
        pos.append(bp[gb[g]] + Rb @ gp[g]); mat.append((Rb @ rr.quat2mat(gq[g]).reshape(3, 3)).ravel())
    sc = rr.scene_from_device(np.array(pos), np.array(mat), m.array("geom_size"), m.array("geom_type"), None, model_hfields(m))
    return _with_meshes(sc, m, surface)


def device_scene(e, m, env, size=None, visible=None, surface=None):
    """the scene of one env from the device's own geom poses"""
    gp, gm = e.get_geom_state(env, 1)
    sc = rr.scene_from_device(gp[0], gm[0], m.array("geom_size") if size is None else size, m.array("geom_type"), visible, model_hfields(m))
    return _with_meshes(sc, m, surface)


# ------------------------------------------------------------------ models
def palette(n, seed=5):
    """n geom colours, float32 numbers in [0.05, 1], alpha not 1 on purpose (it is not used)"""
    rng = np.random.default_rng(seed)
    c = rng.uniform(0.05, 1.0, size=(n, 4)).astype(np.float32).astype(float)
    c[:, 3] = 0.5
    return c


def add_camera(lib, b, name, body, view):
    eye, target, fovy = view
    cid = lib.mjh_builder_add_camera(b, name, body, D(*eye), D(*mat2quat(look_at(eye, target))), fovy)
    assert cid >= 0, lib.mjh_last_error()
    return cid


def add_spec(lib, b, spec, colours=None):
    """a ray_ref spec: static geoms on the world body, every free one on a free body of its own; colours[k] for entry k"""
    for k, g in enumerate(spec):
        if g.get("free"):
            bd = lib.mjh_builder_add_body(b, b"free%d" % k, 0, D(*g["pos"]), D(*g["quat"]), 0.0)
            lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
            gid = lib.mjh_builder_add_geom(b, b"g%d" % k, bd, g["type"], D(*g["size"]), None, None, None, -1, -1, -1, -1)
        else:
            gid = lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, -1, -1, -1)
        assert gid >= 0
        if colours is not None:
            assert lib.mjh_builder_set_geom_rgba(b, gid, D(*colours[k])) == 0, lib.mjh_last_error()


def far_body(lib, b):
    bd = lib.mjh_builder_add_body(b, b"far", 0, D(0, 0, 50.0), None, 0.0)      # (a model needs a moving body; it is out of every view)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"fg", bd, rr.SPHERE, D(0.05, 0, 0), None, None, None, -1, 0, 0, -1)


def compile_model(lib, b):
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m


RIG_CAM_POS = (0.03, 0.01, 0.02)
RIG_CAM_QUAT = tuple(np.array([0.9, 0.2, -0.3, 0.1]) / np.linalg.norm([0.9, 0.2, -0.3, 0.1]))
RIG_RADIUS = 0.12


def prim_model(lib, gravity=(0, 0, 0), rig=False, coloured=True):
    """ray_ref.primitives_spec() in colour with the two static views on the world body; rig: one more free body (a ball) that carries a
    camera inside its own geom"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=list(gravity))
    spec = rr.primitives_spec()
    add_spec(lib, b, spec, palette(len(spec)) if coloured else None)
    add_camera(lib, b, b"front", 0, VIEW_FRONT)
    add_camera(lib, b, b"side", 0, VIEW_SIDE)
    if rig:
        bd = lib.mjh_builder_add_body(b, b"rig", 0, D(0.0, -3.5, 2.5), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        g = lib.mjh_builder_add_geom(b, b"rigg", bd, rr.SPHERE, D(RIG_RADIUS, 0, 0), None, None, None, -1, -1, -1, -1)
        assert g >= 0 and lib.mjh_builder_set_geom_rgba(b, g, D(0.9, 0.4, 0.1, 1.0)) == 0
        assert lib.mjh_builder_add_camera(b, b"eye", bd, D(*RIG_CAM_POS), D(*RIG_CAM_QUAT), 60.0) == 2
    return compile_model(lib, b)


def spheres_model(lib):
    spec = rr.many_spheres_spec()
    assert len(spec) > 64
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, spec, palette(len(spec), seed=6))
    far_body(lib, b)
    add_camera(lib, b, b"above", 0, VIEW_SPHERES)
    return compile_model(lib, b)


def hfield_model(lib):
    b = lib.mjh_builder_create()
    el = (C.c_double * rr.HF_ELEV.size)(*rr.HF_ELEV.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", rr.HF_NROW, rr.HF_NCOL, D(*rr.HF_SIZE), el)
    assert h >= 0
    g = lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*rr.HF_POS), D(*rr.HF_QUAT), None, -1, -1, -1)
    assert g >= 0 and lib.mjh_builder_set_geom_rgba(b, g, D(0.3, 0.7, 0.2, 1.0)) == 0
    far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    add_camera(lib, b, b"cam", 0, VIEW_HFIELD)
    add_camera(lib, b, b"under", 0, VIEW_HFIELD_UNDER)
    return compile_model(lib, b)


def meshes_model(lib):
    """the meshes of tests/test_gpu_ray_tri.py: a torus (tilted, so that the flat top of its hull does not face the way the floor does), a
    jaw and a flat quad over a floor, seen from above — the hull fills the torus's hole and the jaw's gap; the quad has no hull"""
    items = [("torus", (0.0, 0.0, MESH_HEIGHT), TORUS_QUAT, True), ("jaw", (1.1, 0.0, MESH_HEIGHT), None, True), ("flat_quad", (-1.1, 0.0, MESH_HEIGHT), None, True)]
    m, geoms, _ = rt.scene_model(lib, items, camera=(VIEW_MESHES[0], mat2quat(look_at(VIEW_MESHES[0], VIEW_MESHES[1])), VIEW_MESHES[2]))
    return m, geoms


def model_colours(m):
    c = m.array("geom_rgba")
    assert len(c) == 4 * m.ngeom, "the model carries geom_rgba"
    return c.reshape(-1, 4)


# ------------------------------------------------------------------ the comparison
def colour_tolerance(diffuse):
    return 1 + math.ceil(255 * diffuse * math.sqrt(3.0) * TOL_N)


def kept_pixels(name, scene, rays, centre=None):
    """(centre reference (dist, gid, normal, feature), kept [npix], excluded share): asserts the cap"""
    centre = centre if centre is not None else rf.cast(rays[0], rays[1], scene)
    rob, frob = rf.robust_both(rays, scene, centre)
    keep = rob & frob
    share = 1.0 - keep.mean()
    print(f"{name}: {len(keep)} pixels, non-robust share {1.0 - rob.mean():.4f}, excluded share {share:.4f}")
    assert share <= CAP, (name, share)
    return centre, keep, share


def check_render(name, depth, gid, normal, rgba, scene, rays, colours, ambient=0.3, diffuse=0.7, background=(0.0, 0.0, 0.0, 0.0),
                 scale=None, cutoff=0.0, tol_n=TOL_N):
    """ONE env's images against the reference; normal / rgba may be None.  Returns (worst normal error, worst colour difference,
    excluded share)"""
    npix = len(rays[0])
    depth = np.asarray(depth).reshape(npix).astype(float); gid = np.asarray(gid).reshape(npix)
    V = np.asarray(rays[1], float)
    centre, keep, share = kept_pixels(name, scene, rays)
    ref_d, ref_g, ref_n, _ = centre
    if scale is not None:
        ref_d = np.where(ref_g >= 0, ref_d * scale, ref_d)
    if cutoff > 0:
        far = ref_d > cutoff
        ref_d = np.where(far, -1.0, ref_d); ref_g = np.where(far, -1, ref_g); ref_n = np.where(far[:, None], 0.0, ref_n)
        keep = keep & (np.abs(ref_d - cutoff) > 1e-3)
    assert (gid[keep] == ref_g[keep]).all(), name
    hit, khit = gid >= 0, keep & (ref_g >= 0)
    err = np.abs(depth - ref_d) / np.maximum(1.0, np.abs(ref_d))
    assert (depth[~hit] == -1.0).all() and (not khit.any() or err[khit].max() <= TOL), name
    worst_n = worst_c = 0.0
    if normal is not None:
        n = np.asarray(normal).reshape(npix, 3).astype(float)
        assert (n[~hit] == 0.0).all(), f"{name}: a miss has the normal (0, 0, 0)"
        assert np.abs(np.linalg.norm(n[hit], axis=1) - 1.0).max(initial=0.0) <= 1e-6, f"{name}: unit normals"
        assert (np.sum(n[hit] * V[hit], axis=1) <= 1e-6 * np.linalg.norm(V[hit], axis=1)).all(), f"{name}: normals face the camera"
        worst_n = float(np.abs(n[khit] - ref_n[khit]).max(initial=0.0))
    if rgba is not None:
        c = np.asarray(rgba).reshape(npix, 4).astype(int)
        bg = rf.level(np.asarray(background, np.float32))
        assert (c[~hit] == bg).all(), f"{name}: a miss has the background colour exactly"
        assert (c[hit, 3] == 255).all(), name
        ref_c = rf.colour(colours, ref_g, ref_n, V, ambient, diffuse, background).astype(int)
        worst_c = int(np.abs(c[khit] - ref_c[khit]).max(initial=0))
    print(f"{name}: kept hits {int(khit.sum())}, max |n - n_ref| {worst_n:.3e} (TOL_N {tol_n:.1e}), max colour difference {worst_c} (allowed {colour_tolerance(diffuse)})")
    assert worst_n <= tol_n, (name, worst_n)
    assert worst_c <= colour_tolerance(diffuse), (name, worst_c)
    return worst_n, worst_c, share


def flat_colours(colours, gid, background=(0.0, 0.0, 0.0, 0.0)):
    """the image of ambient = 1, diffuse = 0: every hit the level of its geom's colour, every miss the background, bit for bit"""
    gid = np.asarray(gid)
    out = np.tile(rf.level(np.asarray(background, np.float32)), gid.shape + (1,))
    lv = rf.level(np.asarray(colours, float).reshape(-1, 4).astype(np.float32))
    lv[:, 3] = 255
    out[gid >= 0] = lv[gid[gid >= 0]]
    return out.astype(np.uint8)
