"""Depth images on the device (mjh_depth / mjh_depth_device, csrc/depth.hip) against the fp64 references ray_ref.cast / ray_mesh_ref.cast.

The reference casts rays generated in numpy fp64 from the device's own poses: the camera body's pose (mjh_get_body_state) composed with
the model's cam_pos / cam_quat, the geom poses of mjh_get_geom_state.  Only the image arithmetic is under test.  The rule is that of
tests/test_gpu_ray.py: on the pixels robust() accepts the geom ids are equal, misses are exactly -1 and
|depth - ref| <= 5e-5 max(1, ref) — coordinates stay within 8 m, so an fp32 ulp is at most 1e-6, robustness bounds the conditioning
at 10, the fp32 pixel direction displaces the hit point by less than an ulp at these ranges: 1e-5, and the tolerance is five times
that.  At most 2 % of an image's pixels may be non-robust.  Every image is rendered with cull = 1 and cull = 0 and the two must be
the same bits (the contract of the tile cull).

Measured on one MI355X (`pytest tests/test_gpu_depth.py -m gpu -s` prints every case), max scaled error / non-robust share:
primitives, front view 30x20 1.9e-07 / 0, 8x8 1.7e-07 / 0, 9x8 2.7e-07 / 0, 1x1 7.2e-08 / 0, 64x48 2.3e-07 / 0.03 %; side view 30x20 6.2e-07 /
0.17 %, 8x8 3.9e-07 / 1.56 % (one pixel of 64), 9x8 9.2e-08 / 0, 1x1 1.3e-08 / 0; camera on a free body, four poses: own body hidden
3.3e-07 .. 5.7e-07 / 0, from inside its ball 4.4e-08 .. 1.6e-07 / 0; 71 spheres 30x20 6.4e-07 / 0.17 %, 64x48 4.6e-07 / 0.16 %;
tetrahedron field (mesh mode 1) 64x48 5.6e-07 / 0.03 % with 54 mesh geoms named by the reference, 30x20 3.0e-07 / 0; height field
2.6e-07 / 0; mesh model, modes 0 and 1 1.7e-07 / 0; range 2.1e-07, cutoff 1.9e-07, flg_static 1.6e-07, per-env sizes 2.2e-07,
inactive slot 1.9e-07, all / 0.  Worst over all cases 6.4e-07 (bound 5e-05), largest non-robust share 1.56 % (cap 2 %).
"""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr
from helpers import D, set_opt
from mujoco_sim_amd import capi
from mujoco_sim_amd.engine import MjhError
from ray_check import check

pytestmark = pytest.mark.gpu

MJH_ERR_ARG = -1
NENV = 4

# (eye, target, fovy) of the static views
VIEW_FRONT = ((0.2, -4.5, 3.0), (0.0, 0.0, 0.8), 60.0)
VIEW_SIDE = ((3.5, 2.5, 2.2), (0.0, 0.0, 0.8), 45.0)
VIEW_SPHERES = ((0.3, -1.5, 5.5), (0.0, 0.0, 0.6), 55.0)
VIEW_TETRA = ((0.3, -1.5, 6.0), (0.0, 0.0, 0.6), 55.0)
VIEW_HFIELD = ((0.4, -2.2, 1.6), (0.3, -0.2, 0.3), 50.0)
VIEW_MESH = ((0.45, -2.0, 2.6), (0.45, 0.0, 0.6), 50.0)


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


def camera_rays(e, m, cam, env, width, height):
    """world-frame rays of camera `cam` in env `env` from the device's own body pose"""
    xp, xq = e.get_body_state(env, 1)
    b = int(m.array("cam_bodyid")[cam])
    Rb = rr.quat2mat(xq[0, b]).reshape(3, 3)
    pos = xp[0, b] + Rb @ m.array("cam_pos").reshape(-1, 3)[cam]
    R = Rb @ rr.quat2mat(m.array("cam_quat").reshape(-1, 4)[cam]).reshape(3, 3)
    Dc = pixel_dirs(width, height, float(m.array("cam_fovy")[cam]))
    return np.tile(pos, (len(Dc), 1)), Dc @ R.T


def add_camera(lib, b, name, body, view):
    eye, target, fovy = view
    cid = lib.mjh_builder_add_camera(b, name, body, D(*eye), D(*mat2quat(look_at(eye, target))), fovy)
    assert cid >= 0, lib.mjh_last_error()
    return cid


def device_scene(e, m, env, size=None, visible=None, hfield=None, tris=None):
    gp, gm = e.get_geom_state(env, 1)
    sc = rr.scene_from_device(gp[0], gm[0], m.array("geom_size") if size is None else size, m.array("geom_type"), visible, hfield)
    return rm.attach_meshes(sc, m, tris) if tris is not None else sc


def render(e, cam, width, height, **kw):
    """the image with the cull on, after checking that the cull off gives the same bits"""
    d1, g1 = e.depth(cam, width, height, cull=1, **kw)
    d0, g0 = e.depth(cam, width, height, cull=0, **kw)
    assert d1.dtype == np.float32 and g1.dtype == np.int32 and d1.shape == g1.shape == (kw.get("n") or e.nenv - kw.get("env0", 0), height, width)
    assert np.array_equal(d1.view(np.uint32), d0.view(np.uint32)) and np.array_equal(g1, g0), "cull = 1 and cull = 0 give the same bits"
    return d1, g1


# ------------------------------------------------------------------ models
def add_spec(lib, b, spec):
    """a ray_ref spec: static geoms on the world body, every free one on a free body of its own"""
    for k, g in enumerate(spec):
        if g.get("free"):
            bd = lib.mjh_builder_add_body(b, b"free%d" % k, 0, D(*g["pos"]), D(*g["quat"]), 0.0)
            lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, bd, g["type"], D(*g["size"]), None, None, None, -1, -1, -1, -1) >= 0
        else:
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, -1, -1, -1) >= 0


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


def prim_model(lib, gravity=(0, 0, 0), rig=False):
    """ray_ref.primitives_spec() with the two static views on the world body; rig: one more free body (a ball) that carries a camera
    inside its own geom"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=list(gravity))
    add_spec(lib, b, rr.primitives_spec())
    add_camera(lib, b, b"front", 0, VIEW_FRONT)
    add_camera(lib, b, b"side", 0, VIEW_SIDE)
    if rig:
        bd = lib.mjh_builder_add_body(b, b"rig", 0, D(0.0, -3.5, 2.5), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_geom(b, b"rigg", bd, rr.SPHERE, D(RIG_RADIUS, 0, 0), None, None, None, -1, -1, -1, -1) >= 0
        assert lib.mjh_builder_add_camera(b, b"eye", bd, D(*RIG_CAM_POS), D(*RIG_CAM_QUAT), 60.0) == 2
    return compile_model(lib, b)


@pytest.fixture(scope="module")
def prim(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    scene = device_scene(e, m, 0)
    yield m, e, scene
    e.close()


# ------------------------------------------------------------------ 1. every primitive type, static camera, tile edges
@pytest.mark.parametrize("cam", ["front", "side"])
@pytest.mark.parametrize("width,height", [(30, 20), (8, 8), (9, 8), (1, 1)])
def test_primitives(prim, cam, width, height):
    m, e, scene = prim
    depth, gid = render(e, cam, width, height)
    rays = camera_rays(e, m, m.name2id(5, cam), 0, width, height)
    for env in range(NENV):      # no per-env data: every env sees the same scene
        check(f"primitives {cam} {width}x{height} env {env}", depth[env], gid[env], scene, rays)
    if (width, height) == (30, 20):
        assert {int(scene["type"][g]) for g in gid[0].ravel() if g >= 0} >= {rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.ELLIPSOID, rr.CYLINDER, rr.BOX}
        d2, g2 = e.depth(m.name2id(5, cam), width, height)      # by id, the default options
        assert np.array_equal(d2, depth) and np.array_equal(g2, gid)


def test_primitives_larger_image(prim):
    m, e, scene = prim
    depth, gid = render(e, "front", 64, 48, n=1)
    check("primitives front 64x48", depth[0], gid[0], scene, camera_rays(e, m, 0, 0, 64, 48))


# ------------------------------------------------------------------ 2. a camera on a free body, its own pose in every env
@pytest.fixture(scope="module")
def rig(lib):
    m = prim_model(lib, rig=True)
    e = ms.Engine(m, NENV)
    rng = np.random.default_rng(23)
    bd = m.name2id(0, "rig")
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[bd]])
    q = np.tile(m.array("qpos0"), (NENV, 1))
    Rc = rr.quat2mat(RIG_CAM_QUAT).reshape(3, 3)
    for i in range(NENV):
        eye = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-4.2, -3.2), rng.uniform(2.0, 3.2)])
        Rw = look_at(eye, np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.4, 0.4, size=3))
        roll = rng.uniform(-0.6, 0.6)
        Rw = Rw @ np.array([[np.cos(roll), -np.sin(roll), 0], [np.sin(roll), np.cos(roll), 0], [0, 0, 1.0]])
        Rb = Rw @ Rc.T
        q[i, adr:adr + 3] = eye - Rb @ np.array(RIG_CAM_POS)
        q[i, adr + 3:adr + 7] = mat2quat(Rb)
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv)))
    e.forward()
    yield m, e, bd
    e.close()


def test_camera_on_a_free_body(rig):
    m, e, bd = rig
    width, height = 30, 20
    body = m.array("geom_bodyid")
    rigg = int(np.nonzero(body == bd)[0][0])
    depth, gid = render(e, "eye", width, height, bodyexclude=bd)
    inside_d, inside_g = render(e, "eye", width, height)
    xp, _ = e.get_body_state()
    assert np.abs(xp[0, bd] - xp[1, bd]).max() > 0.1, "every env has its own camera pose"
    for env in range(NENV):
        rays = camera_rays(e, m, 2, env, width, height)
        check(f"rig env {env} (own body hidden)", depth[env], gid[env], device_scene(e, m, env, visible=body != bd), rays)
        assert (gid[env] >= 0).mean() > 0.3 and not (gid[env] == rigg).any()
        # the camera sits inside its body's ball: every pixel sees the ball's far surface
        check(f"rig env {env} (from inside)", inside_d[env], inside_g[env], device_scene(e, m, env), rays)
        assert (inside_g[env] == rigg).all() and inside_d[env].max() < 2 * RIG_RADIUS
    assert not np.array_equal(depth[0], depth[1])


# ------------------------------------------------------------------ 3. more geoms than one staging pass holds
@pytest.fixture(scope="module")
def spheres(lib):
    spec = rr.many_spheres_spec()
    assert len(spec) > 64
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, spec)
    far_body(lib, b)
    add_camera(lib, b, b"above", 0, VIEW_SPHERES)
    m = compile_model(lib, b)
    e = ms.Engine(m, NENV)
    yield m, e, device_scene(e, m, 0)
    e.close()


@pytest.mark.parametrize("width,height", [(30, 20), (64, 48)])
def test_more_geoms_than_one_staging_pass(spheres, width, height):
    m, e, scene = spheres
    depth, gid = render(e, "above", width, height)
    for env in range(1, NENV):
        assert np.array_equal(depth[env], depth[0]) and np.array_equal(gid[env], gid[0])
    check(f"many spheres {width}x{height}", depth[0], gid[0], scene, camera_rays(e, m, 0, 0, width, height))
    assert (gid[0] >= 64).any() and ((gid[0] >= 0) & (gid[0] < 64)).any(), "geoms of both staging passes are seen"


@pytest.mark.parametrize("ngeom", [65, 130])
def test_staging_pass_edges(lib, ngeom):
    """65 geoms: the second staging pass holds a single candidate; 130: a third pass follows a full second one.  The camera stands over
    the last sphere; 9 x 8 pixels: tiles partial in both directions"""
    spec, last = rr.pass_edge_spec(ngeom)
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, spec)
    add_camera(lib, b, b"over", 0, ((last[0] + 0.3, last[1] - 0.8, 3.0), (last[0] - 0.25, last[1] - 0.15, 0.5), 45.0))
    m = compile_model(lib, b)
    assert m.ngeom == ngeom
    e = ms.Engine(m, NENV)
    depth, gid = render(e, "over", 9, 8)      # (cull 0 and cull 1: the same bits)
    for env in range(1, NENV):
        assert np.array_equal(depth[env], depth[0]) and np.array_equal(gid[env], gid[0])
    check(f"{ngeom} geoms 9x8", depth[0], gid[0], device_scene(e, m, 0), camera_rays(e, m, 0, 0, 9, 8))
    assert (gid[0] == ngeom - 1).any(), "the last geom, in the last pass, is seen"
    assert all(((gid[0] >= 64 * p) & (gid[0] < 64 * (p + 1))).any() for p in range((ngeom + 63) // 64)), "geoms of every staging pass are seen"
    e.close()


@pytest.fixture(scope="module")
def tetra(lib):
    spec = rm.tetra_field_spec()
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    v = np.ascontiguousarray(0.4 * rm.tetra_points(), float)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    assert mid >= 0
    for k, g in enumerate(spec):
        if g["type"] == rr.MESH:
            assert lib.mjh_builder_add_mesh_geom(b, b"g%d" % k, 0, mid, D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
        else:
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
    far_body(lib, b)
    add_camera(lib, b, b"above", 0, VIEW_TETRA)
    m = compile_model(lib, b)
    e = ms.Engine(m, NENV)
    e.ray_mesh_mode = 1
    tris = [rm.hull_triangles(x) for x in rm.model_mesh_verts(m)]
    yield m, e, device_scene(e, m, 0, tris=tris)
    e.close()


def test_tetrahedron_field_in_mesh_mode_1(tetra):
    m, e, scene = tetra
    assert m.ngeom == 107 and (m.array("geom_type") == rr.MESH).sum() == 70
    width, height = 64, 48
    depth, gid = render(e, "above", width, height)
    for env in range(1, NENV):
        assert np.array_equal(depth[env], depth[0]) and np.array_equal(gid[env], gid[0])
    rays = camera_rays(e, m, 0, 0, width, height)
    check("tetrahedron field 64x48", depth[0], gid[0], scene, rays)
    _, ref_g = rm.cast(rays[0], rays[1], scene)
    types = m.array("geom_type")
    assert len({int(g) for g in ref_g if g >= 0 and types[g] == rr.MESH}) >= 10, "the reference names at least ten different mesh geoms"
    assert (gid[0] >= 64).any() and ((gid[0] >= 0) & (gid[0] < 64)).any()
    d30, g30 = render(e, "above", 30, 20, n=1)
    check("tetrahedron field 30x20", d30[0], g30[0], scene, camera_rays(e, m, 0, 0, 30, 20))


# ------------------------------------------------------------------ 5. height field
def test_hfield(lib):
    import hfield_ref
    b = lib.mjh_builder_create()
    el = (C.c_double * rr.HF_ELEV.size)(*rr.HF_ELEV.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", rr.HF_NROW, rr.HF_NCOL, D(*rr.HF_SIZE), el)
    assert h >= 0
    assert lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*rr.HF_POS), D(*rr.HF_QUAT), None, -1, -1, -1) >= 0
    far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    add_camera(lib, b, b"cam", 0, VIEW_HFIELD)
    m = compile_model(lib, b)
    e = ms.Engine(m, NENV)
    scene = device_scene(e, m, 0, hfield={0: hfield_ref.hfield_of(m, 0)})
    depth, gid = render(e, "cam", 30, 20)
    rays = camera_rays(e, m, 0, 0, 30, 20)
    for env in range(NENV):
        check(f"hfield env {env}", depth[env], gid[env], scene, rays)
    assert (gid[0] == 0).mean() > 0.3
    e.close()


# ------------------------------------------------------------------ 6. mesh mode
def test_mesh_mode(lib, prim):
    # ray_ref.mesh_model's scene (a floor, two free bodies with a box-shaped mesh geom each, a static ball), with a camera
    b = lib.mjh_builder_create()
    v = np.ascontiguousarray(np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * [0.2, 0.15, 0.1])
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    assert mid >= 0
    lib.mjh_builder_add_geom(b, b"floor", 0, rr.PLANE, D(0, 0, 0.05), None, None, None, -1, -1, -1, -1)
    for k in range(2):
        bd = lib.mjh_builder_add_body(b, b"m%d" % k, 0, D(0.9 * k, 0, 1.0), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, bd, mid, None, None, None, -1, -1, -1, -1) >= 0
    lib.mjh_builder_add_geom(b, b"ball", 0, rr.SPHERE, D(0.2, 0, 0), D(0, 0, 0.4), None, None, -1, -1, -1, -1)
    add_camera(lib, b, b"cam", 0, VIEW_MESH)
    m = compile_model(lib, b)
    e = ms.Engine(m, NENV)
    mesh = np.nonzero(m.array("geom_type") == rr.MESH)[0]
    rays = camera_rays(e, m, 0, 0, 30, 20)
    assert e.ray_mesh_mode == 0
    d0, g0 = render(e, "cam", 30, 20)
    check("mesh model, mode 0", d0[0], g0[0], device_scene(e, m, 0), rays)      # (the reference without the meshes)
    assert not np.isin(g0, mesh).any()
    e.ray_mesh_mode = 1
    d1, g1 = render(e, "cam", 30, 20)
    tris = [rm.hull_triangles(x) for x in rm.model_mesh_verts(m)]
    check("mesh model, mode 1", d1[0], g1[0], device_scene(e, m, 0, tris=tris), rays)
    assert all((g1[0] == g).sum() >= 4 for g in mesh), "both meshes are seen"
    e.ray_mesh_mode = 0
    d2, g2 = e.depth("cam", 30, 20)
    assert np.array_equal(d2, d0) and np.array_equal(g2, g0)
    e.close()
    # a model without meshes: mode 1 is mode 0, bit for bit
    pm, pe, _ = prim
    a = pe.depth("front", 30, 20)
    pe.ray_mesh_mode = 1
    try:
        c = pe.depth("front", 30, 20)
    finally:
        pe.ray_mesh_mode = 0
    assert np.array_equal(a[0].view(np.uint32), c[0].view(np.uint32)) and np.array_equal(a[1], c[1])


# ------------------------------------------------------------------ 7. options
def test_range_and_cutoff(prim):
    m, e, scene = prim
    width, height = 30, 20
    rays = camera_rays(e, m, 0, 0, width, height)
    norm = np.linalg.norm(rays[1], axis=1)
    d0, g0 = render(e, "front", width, height, n=1)
    dr, gr = render(e, "front", width, height, n=1, range=1)
    check("range 1", dr[0], gr[0], scene, rays, scale=norm)
    assert np.array_equal(gr, g0) and (dr[0].ravel()[g0[0].ravel() >= 0] >= d0[0].ravel()[g0[0].ravel() >= 0]).all()
    ref_d, ref_g = rm.cast(rays[0], rays[1], scene)
    cut = 0.5 * (ref_d[ref_g >= 0].min() + ref_d[ref_g >= 0].max())
    dc, gc = render(e, "front", width, height, n=1, cutoff=cut)
    check("cutoff", dc[0], gc[0], scene, rays, cutoff=cut)
    far = d0[0] > np.float32(cut)
    assert far.any() and (g0[0][~far] >= 0).any()
    assert (dc[0][far] == -1.0).all() and (gc[0][far] == -1).all()
    assert np.array_equal(dc[0][~far].view(np.uint32), d0[0][~far].view(np.uint32)) and np.array_equal(gc[0][~far], g0[0][~far]), "the rest is unchanged"
    # the far plane applies to the reported value: with range = 1 to the distance
    cut_r = 0.5 * ((ref_d * norm)[ref_g >= 0].min() + (ref_d * norm)[ref_g >= 0].max())
    dcr, gcr = render(e, "front", width, height, n=1, range=1, cutoff=cut_r)
    far_r = dr[0] > np.float32(cut_r)
    assert far_r.any() and (dcr[0][far_r] == -1.0).all() and (gcr[0][far_r] == -1).all()
    assert np.array_equal(dcr[0][~far_r].view(np.uint32), dr[0][~far_r].view(np.uint32))


def test_flg_static(prim):
    m, e, scene = prim
    body = m.array("geom_bodyid")
    d, g = render(e, "front", 30, 20, n=1, flg_static=0)
    check("flg_static 0", d[0], g[0], dict(scene, visible=body != 0), camera_rays(e, m, 0, 0, 30, 20))
    assert (body[g[0][g[0] >= 0]] != 0).all() and (g[0] >= 0).any()


def test_per_env_geom_sizes(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    size = m.array("geom_size")
    small = (0.8 * size).astype(np.float32).astype(float)
    e.set_env_param("geom_size", small[None, :], env0=1)
    depth, gid = render(e, "front", 30, 20)
    rays = camera_rays(e, m, 0, 0, 30, 20)
    for env in range(NENV):
        check(f"per-env sizes env {env}", depth[env], gid[env], device_scene(e, m, env, size=small if env == 1 else size), rays)
    assert not np.array_equal(depth[1], depth[0]) and np.array_equal(depth[2], depth[0]) and np.array_equal(depth[3], depth[0])
    e.close()


def test_inactive_slot_hides_its_body_in_that_env_only(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    body = m.array("geom_bodyid")
    d0, g0 = render(e, "front", 30, 20)
    seen = [int(g) for g in np.unique(g0[0]) if g >= 0 and body[g] > 0]
    g = max(seen, key=lambda k: int((g0[0] == k).sum())); bd = int(body[g])
    e.set_slot_active(bd, 0, env0=2, n=1)
    d1, g1 = render(e, "front", 30, 20)
    assert not (g1[2] == g).any() and (g1[0] == g).any()
    for env in (0, 1, 3):
        assert np.array_equal(d1[env], d0[env]) and np.array_equal(g1[env], g0[env])
    check("inactive slot", d1[2], g1[2], device_scene(e, m, 2, visible=body != bd), camera_rays(e, m, 0, 2, 30, 20))
    e.set_slot_active(bd, 1, env0=2, n=1)
    d2, g2 = e.depth("front", 30, 20)
    assert np.array_equal(d2, d0) and np.array_equal(g2, g0)
    e.close()


# ------------------------------------------------------------------ 8. the device form
def test_depth_device_same_bits(rig):
    import torch
    m, e, bd = rig
    width, height, env0, n = 30, 20, 1, 3
    depth, gid = e.depth("eye", width, height, env0=env0, n=n, bodyexclude=bd)
    dev = torch.device("cuda:0")
    td = torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev); tg = torch.full((n, height, width), 7, dtype=torch.int32, device=dev)
    t2 = torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.depth_device(td.data_ptr(), tg.data_ptr(), "eye", width, height, env0=env0, n=n, bodyexclude=bd)
    e.depth_device(t2.data_ptr(), None, 2, width, height, env0=env0, n=n, bodyexclude=bd)
    e.synchronize()
    assert np.array_equal(td.cpu().numpy().view(np.uint32), depth.view(np.uint32)) and np.array_equal(tg.cpu().numpy(), gid)
    assert np.array_equal(t2.cpu().numpy().view(np.uint32), depth.view(np.uint32)), "without a geomid image the depth bits are the same"
    only_d = np.full((n, height, width), 7.0, dtype=np.float32)
    o = capi.DepthOptions(); e.lib.mjh_depth_default_options(C.byref(o))
    assert (o.camera, o.width, o.height, o.bodyexclude, o.flg_static, o.range, o.cull, o.cutoff) == (0, 64, 64, -1, 1, 0, 1, 0.0)
    o.camera, o.width, o.height, o.bodyexclude = 2, width, height, bd
    assert e.lib.mjh_depth(e.h, env0, n, C.byref(o), C.c_void_p(only_d.ctypes.data), None) == 0
    assert np.array_equal(only_d.view(np.uint32), depth.view(np.uint32))


# ------------------------------------------------------------------ 9. nothing of the state is written
def _snapshot(e):
    t, q, v, w = e.get_state()
    return [t, q, v, w, e.get_stats(), e.get_field("qacc"), e.get_field("qfrc_applied")]


def test_no_side_effects(lib):
    m = prim_model(lib, gravity=(0, 0, -9.81))
    a, b = ms.Engine(m, NENV), ms.Engine(m, NENV)
    a.step(150); b.step(150)      # (the free bodies have begun to land on the floor)
    before = _snapshot(a)
    a.depth("front", 30, 20); a.depth("side", 9, 8, env0=1, n=2, cull=0, range=1)
    for x, y in zip(before, _snapshot(a)):
        assert np.array_equal(x, y)
    a.step(3); b.step(3)
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "a step after a depth call equals a step without one"
    # ... and between the halves of a split step, as mjh_ray
    a.step1(); d, g = a.depth("front", 30, 20); a.step2()
    b.step1(); b.get_geom_state(0, NENV); b.step2()
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "the call sequence rules are those of mjh_get_geom_state"
    assert (g >= 0).any()
    a.close(); b.close()


# ------------------------------------------------------------------ 10. errors
def test_errors_launch_nothing(prim, lib):
    m, e, scene = prim
    width, height = 9, 8
    good_d, good_g = e.depth("front", width, height)
    depth = np.full((NENV, height, width), 7.0, dtype=np.float32); gid = np.full((NENV, height, width), 7, dtype=np.int32)

    def call(eng=e, env0=0, n=NENV, null=False, **kw):
        o = capi.DepthOptions(); lib.mjh_depth_default_options(C.byref(o))
        o.width, o.height = width, height
        for k, v in kw.items():
            setattr(o, k, v)
        return lib.mjh_depth(eng.h, env0, n, C.byref(o), None if null else C.c_void_p(depth.ctypes.data), C.c_void_p(gid.ctypes.data))

    def ok():
        assert (depth == 7.0).all() and (gid == 7).all(), "nothing was launched: the outputs are untouched"
        assert call() == 0
        assert np.array_equal(depth, good_d) and np.array_equal(gid, good_g)
        depth[:] = 7.0; gid[:] = 7

    for bad in (dict(camera=2), dict(camera=-1), dict(bodyexclude=m.nbody), dict(bodyexclude=-2), dict(width=0), dict(height=0), dict(width=-3),
                dict(env0=2, n=3), dict(env0=-1, n=2), dict(env0=NENV, n=1), dict(n=0), dict(null=True), dict(width=1 << 16, height=1 << 15)):
        assert call(**bad) == MJH_ERR_ARG, bad
        assert lib.mjh_last_error()
        ok()
    assert lib.mjh_depth_device(e.h, 0, NENV, None, None, None) == MJH_ERR_ARG
    ok()
    with pytest.raises(MjhError):
        e.depth("front", 0, 8)
    with pytest.raises(ValueError):
        e.depth("no such camera", 8, 8)
    with pytest.raises(TypeError):
        e.depth("front", 8, 8, per_env=1)
    ok()
    # a model without cameras
    s = ms.scene("s24"); es = ms.Engine(s, NENV)
    assert s.ncam == 0 and call(eng=es) == MJH_ERR_ARG and b"camera" in lib.mjh_last_error()
    assert (depth == 7.0).all() and (gid == 7).all()
    es.step(2)      # (and the engine goes on as usual)
    es.close()
    ok()
