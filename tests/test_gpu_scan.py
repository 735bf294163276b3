"""Lidar range images on the device (mjh_scan / mjh_scan_device, csrc/scan.hip) against the fp64 references ray_ref.cast /
ray_mesh_ref.cast.

The reference casts beams generated in numpy fp64 from the interface's formula d = (cos el cos az, cos el sin az, sin el) at the
device's own site pose: the site body's pose (mjh_get_body_state) composed with the model's site_pos / site_quat, and against the geom
poses of mjh_get_geom_state.  Only the scan arithmetic is under test.  The rule is ray_check.check's, the project's: on the beams
robust() accepts the geom ids are equal, misses are exactly -1 and |range - ref| <= 5e-5 max(1, ref); at most 2 % of a scan's beams
may be non-robust.  The sensors stand where the reference alone finds at most 1 % of the beams non-robust (computed on the CPU from
the models' initial poses before anything ran on a GPU; the share of every case is printed).  Every scan is cast with cull = 1 and
cull = 0 and the two must be the same bits (the contract of the tile cull).

Measured on one MI355X (`pytest tests/test_gpu_scan.py -m gpu -s` prints every case), max scaled error / non-robust share: primitives
1 x 1 8.2e-08 / 0, planar 1 x 1081 2.0e-07 / 0.09 %, full turn 16 x 360 4.3e-07 / 0.12 %, 5 x 3 4.7e-08 / 0, 9 x 70 3.1e-07 / 0, the
unordered table 2.3e-07 / 0.16 %, world frame 1.8e-07 / 0; sensor on a free body, four poses: own body hidden 2.5e-07 .. 5.0e-07 / 0,
from inside its ball 7.9e-08 .. 8.5e-08 / 0; 71 spheres 5.6e-07 / 0.20 %; tetrahedron field (mesh mode 1) 1.8e-07 / 0.39 %; mesh
surface 1 4.8e-07 / 0; height field 2.9e-07 / 0.26 %; cutoff, flg_static, inactive slot 4.3e-07 / at most 0.12 %; points within 1.0e-07
of range d64; against mjh_ray fed the same beams 5.4e-07 (full turn, 5181 of 5760 ranges bitwise equal) and 2.4e-07 (planar, 1038 of
1081).  Worst over all cases 5.6e-07 (bound 5e-05), largest non-robust share 0.39 % (cap 2 %)."""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr
import ray_tri_ref as rt
import scan_ref as sr
from helpers import D, set_opt
from mujoco_sim_amd import capi
from mujoco_sim_amd.engine import MjhError
from ray_check import TOL, check

pytestmark = pytest.mark.gpu

MJH_ERR_ARG = -1
NENV = 4
DEG = sr.DEG


def unit(q):
    return tuple(np.asarray(q, float) / np.linalg.norm(q))


def yaw(a):
    return (np.cos(a / 2), 0.0, 0.0, np.sin(a / 2))


# the sensors: (site_pos, site_quat) in their body.  In the middle of the primitives, tilted; the others upright (turned about z only):
# their floors are unbounded, and a tilted row would graze them
PRIM_SENSOR = ((0.1, 0.2, 1.0), unit((0.98, 0.05, -0.08, 0.15)))
RIG_SENSOR = ((0.03, 0.01, 0.02), unit((0.9, 0.2, -0.3, 0.1)))
RIG_RADIUS = 0.12
SPHERES_SENSOR = ((0.0, 0.225, 0.75), yaw(0.3))
TETRA_SENSOR = ((0.0, 0.225, 0.75), yaw(-0.7))
HFIELD_SENSOR = ((0.3, -0.2, 1.3), yaw(1.1))
TRI_SENSOR = ((0.0, 0.0, 1.0), yaw(0.4))
# their patterns beside scan_ref.PATTERNS: full turns whose rows stay off the horizon
SPHERES_PATTERN = (128, 8, -np.pi, 2 * np.pi / 128, (-57.0 * DEG, 10.0 * DEG))
TETRA_PATTERN = (128, 8, -np.pi, 2 * np.pi / 128, (-57.0 * DEG, 10.0 * DEG))
HFIELD_PATTERN = (64, 6, -np.pi, 2 * np.pi / 64, (-85.0 * DEG, 10.0 * DEG))
TRI_PATTERN = (96, 8, -np.pi, 2 * np.pi / 96, (-47.0 * DEG, 12.0 * DEG))
RIG_PATTERN = sr.PATTERNS["9x70"]
WORLD_PATTERN = (90, 6, -np.pi, 2 * np.pi / 90, (12.0 * DEG, 9.0 * DEG))


# ------------------------------------------------------------------ the sensor's beams in fp64
def sensor_rays(e, m, site, env, pattern):
    """world-frame (origins, unit directions) of the pattern's beams from site `site` in env `env`, from the device's own body pose"""
    xp, xq = e.get_body_state(env, 1)
    b = int(m.array("site_bodyid")[site])
    Rb = rr.quat2mat(xq[0, b]).reshape(3, 3)
    pos = xp[0, b] + Rb @ m.array("site_pos").reshape(-1, 3)[site]
    R = Rb @ rr.quat2mat(m.array("site_quat").reshape(-1, 4)[site]).reshape(3, 3)
    Ds = sr.beams64(pattern).reshape(-1, 3)
    return np.tile(pos, (len(Ds), 1)), Ds @ R.T


def device_scene(e, m, env, visible=None, hfield=None, tris=None):
    gp, gm = e.get_geom_state(env, 1)
    sc = rr.scene_from_device(gp[0], gm[0], m.array("geom_size"), m.array("geom_type"), visible, hfield)
    return rm.attach_meshes(sc, m, tris) if tris is not None else sc


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def scan(e, site, pattern, **kw):
    """the scan with the cull on, after checking that the cull off gives the same bits"""
    r1, g1 = e.scan(site, **sr.scan_kwargs(pattern), cull=1, **kw)
    r0, g0 = e.scan(site, **sr.scan_kwargs(pattern), cull=0, **kw)
    assert r1.dtype == np.float32 and g1.dtype == np.int32 and r1.shape == g1.shape == (kw.get("n") or e.nenv - kw.get("env0", 0), pattern[1], pattern[0])
    assert np.array_equal(bits(r1), bits(r0)) and np.array_equal(g1, g0), "cull = 1 and cull = 0 give the same bits"
    return r1, g1


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
    bd = lib.mjh_builder_add_body(b, b"far", 0, D(0, 0, 50.0), None, 0.0)      # (a model needs a moving body; it is above every beam)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"fg", bd, rr.SPHERE, D(0.05, 0, 0), None, None, None, -1, 0, 0, -1)


def add_site(lib, b, name, body, sensor):
    sid = lib.mjh_builder_add_site(b, name, body, D(*sensor[0]), D(*sensor[1]))
    assert sid >= 0, lib.mjh_last_error()
    return sid


def compile_model(lib, b):
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m


def prim_model(lib, gravity=(0, 0, 0), rig=False):
    """ray_ref.primitives_spec() with the sensor `lidar` on the world body in the middle of them; rig: one more free body (a ball) that
    carries the sensor `head` inside its own geom"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=list(gravity))
    add_spec(lib, b, rr.primitives_spec())
    add_site(lib, b, b"lidar", 0, PRIM_SENSOR)
    if rig:
        bd = lib.mjh_builder_add_body(b, b"rig", 0, D(0.0, -1.2, 1.4), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_geom(b, b"rigg", bd, rr.SPHERE, D(RIG_RADIUS, 0, 0), None, None, None, -1, -1, -1, -1) >= 0
        assert add_site(lib, b, b"head", bd, RIG_SENSOR) == 1
    return compile_model(lib, b)


def rig_qpos(m, nenv=NENV):
    """a pose of the rig per env: in front of, above and among the primitives, at a random orientation"""
    rng = np.random.default_rng(29)
    bd = m.name2id(0, "rig")
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[bd]])
    q = np.tile(m.array("qpos0"), (nenv, 1))
    for i in range(nenv):
        q[i, adr:adr + 3] = [rng.uniform(-1.2, 1.2), rng.uniform(-1.4, -0.2), rng.uniform(1.0, 1.8)]
        q[i, adr + 3:adr + 7] = rr.random_quat(rng)
    return q


def spheres_model(lib):
    spec = rr.many_spheres_spec()
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, spec)
    far_body(lib, b)
    add_site(lib, b, b"lidar", 0, SPHERES_SENSOR)
    return compile_model(lib, b)


def tetra_model(lib):
    """ray_mesh_ref.tetra_field_spec(): 70 tetrahedron-mesh geoms of one asset and 35 spheres over a floor, the sensor among them"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    v = np.ascontiguousarray(0.4 * rm.tetra_points(), float)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    assert mid >= 0
    for k, g in enumerate(rm.tetra_field_spec()):
        if g["type"] == rr.MESH:
            assert lib.mjh_builder_add_mesh_geom(b, b"g%d" % k, 0, mid, D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
        else:
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
    far_body(lib, b)
    add_site(lib, b, b"lidar", 0, TETRA_SENSOR)
    return compile_model(lib, b)


def hfield_model(lib):
    b = lib.mjh_builder_create()
    el = (C.c_double * rr.HF_ELEV.size)(*rr.HF_ELEV.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", rr.HF_NROW, rr.HF_NCOL, D(*rr.HF_SIZE), el)
    assert h >= 0
    assert lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*rr.HF_POS), D(*rr.HF_QUAT), None, -1, -1, -1) >= 0
    far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    add_site(lib, b, b"lidar", 0, HFIELD_SENSOR)
    return compile_model(lib, b)


TRI_ITEMS = [("torus", (0.9, 0.1, 1.0), unit((0.8, 0.5, 0.2, 0.1)), False), ("jaw", (-0.8, 0.3, 0.9), unit((0.3, 0.1, -0.2, 0.9)), False),
             ("box12", (0.1, 1.0, 0.8), None, False), ("sheet", (0.0, -0.9, 0.7), unit((0.9, 0.3, 0.1, 0.0)), True)]


def tri_model(lib):
    """meshes with triangle tables around a sensor on the world body (item 0 is static: its body is the world)"""
    return rt.scene_model(lib, TRI_ITEMS, site=(0, *TRI_SENSOR))[0]


@pytest.fixture(scope="module")
def prim(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    yield m, e, device_scene(e, m, 0)
    e.close()


# ------------------------------------------------------------------ 1. every primitive type around the sensor, every pattern
@pytest.mark.parametrize("name", list(sr.PATTERNS))
def test_primitives(prim, name):
    m, e, scene = prim
    pattern = sr.PATTERNS[name]
    rng_, gid = scan(e, "lidar", pattern)
    for env in range(1, NENV):      # no per-env data: every env sees the same scene
        assert np.array_equal(bits(rng_[env]), bits(rng_[0])) and np.array_equal(gid[env], gid[0])
    check(f"primitives {name}", rng_[0], gid[0], scene, sensor_rays(e, m, 0, 0, pattern))
    if name == "full turn 16x360":
        assert {int(scene["type"][g]) for g in gid[0].ravel() if g >= 0} >= {rr.SPHERE, rr.CAPSULE, rr.ELLIPSOID, rr.CYLINDER, rr.BOX}
        r2, g2 = e.scan(0, **sr.scan_kwargs(pattern))      # by id, the default options
        assert np.array_equal(bits(r2), bits(rng_)) and np.array_equal(g2, gid)
    if name == "table 9x70":
        assert (gid[0][1] == 0).mean() > 0.5, "the row at -80 degrees looks at the floor"
        assert (gid[0][4] == -1).all(), "the row at +80 degrees at the sky"


def test_world_frame_and_default_pattern(prim, lib):
    """site -1 is the world frame; the default options are one planar turn in 1-degree steps"""
    m, e, scene = prim
    o = capi.ScanOptions(); lib.mjh_scan_default_options(C.byref(o))
    assert (o.site, o.width, o.height, o.bodyexclude, o.flg_static, o.cull, o.cutoff) == (-1, 360, 1, -1, 1, 1, 0.0) and not o.elevation
    assert o.azimuth0 == -np.pi and o.azimuth_step == 2 * np.pi / 360 and o.elevation0 == 0.0 and o.elevation_step == 0.0
    # (the world's origin lies in the floor: the static geoms are hidden and the rows look up at the free bodies)
    r, g = scan(e, None, WORLD_PATTERN, n=1, flg_static=0)
    Ds = sr.beams64(WORLD_PATTERN).reshape(-1, 3)
    check("world frame", r[0], g[0], dict(scene, visible=m.array("geom_bodyid") != 0), (np.zeros_like(Ds), Ds))
    assert (g[0] >= 0).sum() >= 20


# ------------------------------------------------------------------ 2. points
@pytest.mark.parametrize("name", ["full turn 16x360", "planar 1x1081", "table 9x70"])
def test_points(prim, name):
    m, e, scene = prim
    pattern = sr.PATTERNS[name]
    r, g = e.scan("lidar", **sr.scan_kwargs(pattern), n=2)
    r3, g3, pts = e.scan("lidar", **sr.scan_kwargs(pattern), n=2, points=True)
    assert pts.dtype == np.float32 and pts.shape == r.shape + (3,)
    assert np.array_equal(bits(r3), bits(r)) and np.array_equal(g3, g), "range and geom id are the same bits with and without the points pointer"
    d64 = sr.beams64(pattern)[None]
    miss = g3 < 0
    assert miss.any() and (~miss).any()
    assert (pts[miss] == 0.0).all(), "a miss is the origin"
    err = np.abs(pts.astype(float) - r3.astype(float)[..., None] * d64).max(axis=-1)
    worst = (err / np.maximum(1.0, r3.astype(float)))[~miss].max()
    print(f"points {name}: max scaled error {worst:.3e}")
    assert worst <= TOL


# ------------------------------------------------------------------ 3. against mjh_ray fed the same beams
@pytest.mark.parametrize("name", ["full turn 16x360", "planar 1x1081"])
def test_against_the_ray_route(prim, name):
    m, e, scene = prim
    pattern = sr.PATTERNS[name]
    r, g = e.scan("lidar", **sr.scan_kwargs(pattern), n=1)
    Ds = sr.beams64(pattern).reshape(-1, 3)
    dist, gid = e.ray(np.zeros_like(Ds), Ds, site=0, n=1)
    rob = rm.robust(sensor_rays(e, m, 0, 0, pattern), scene)
    r0, g0 = r[0].ravel(), g[0].ravel()
    assert (g0[rob] == gid[0][rob]).all()
    err = np.abs(r0.astype(float) - dist[0]) / np.maximum(1.0, np.abs(dist[0]))
    same = np.array_equal(r0, dist[0].astype(np.float32)) and np.array_equal(g0, gid[0])
    print(f"ray route {name}: robust share {rob.mean():.4f}, max scaled difference {err[rob].max():.3e}, bitwise equal: {same} "
          f"({int((r0 == dist[0].astype(np.float32)).sum())} of {len(r0)} ranges)")
    assert err[rob].max() <= TOL


# ------------------------------------------------------------------ 4. a sensor on a free body, its own pose in every env
@pytest.fixture(scope="module")
def rig(lib):
    m = prim_model(lib, rig=True)
    e = ms.Engine(m, NENV)
    e.set_state(qpos=rig_qpos(m), qvel=np.zeros((NENV, m.nv)))
    e.forward()
    yield m, e, m.name2id(0, "rig")
    e.close()


def test_sensor_on_a_free_body(rig):
    m, e, bd = rig
    body = m.array("geom_bodyid")
    rigg = int(np.nonzero(body == bd)[0][0])
    r, g = scan(e, "head", RIG_PATTERN, bodyexclude=bd)
    ri, gi = scan(e, "head", RIG_PATTERN)
    xp, _ = e.get_body_state()
    assert np.abs(xp[0, bd] - xp[1, bd]).max() > 0.1, "every env has its own sensor pose"
    for env in range(NENV):
        rays = sensor_rays(e, m, 1, env, RIG_PATTERN)
        check(f"rig env {env} (own body hidden)", r[env], g[env], device_scene(e, m, env, visible=body != bd), rays)
        assert not (g[env] == rigg).any()
        # the sensor sits inside its body's ball: every beam sees the ball's far surface
        check(f"rig env {env} (from inside)", ri[env], gi[env], device_scene(e, m, env), rays)
        assert (gi[env] == rigg).all() and ri[env].max() < 2 * RIG_RADIUS
    assert not np.array_equal(r[0], r[1]) and (g >= 0).mean() > 0.1


def test_scan_device_same_bits(rig):
    import torch
    m, e, bd = rig
    pattern = sr.PATTERNS["table 9x70"]
    width, height = pattern[:2]
    env0, n = 1, 3
    kw = dict(sr.scan_kwargs(pattern), env0=env0, n=n, bodyexclude=bd)
    r, g, pts = e.scan("head", points=True, **kw)
    dev = torch.device("cuda:0")
    tr = torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev); tg = torch.full((n, height, width), 7, dtype=torch.int32, device=dev)
    tp = torch.full((n, height, width, 3), 7.0, dtype=torch.float32, device=dev); t2 = torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.scan_device(tr.data_ptr(), tg.data_ptr(), tp.data_ptr(), "head", **kw)
    e.scan_device(t2.data_ptr(), None, None, 1, **kw)
    e.synchronize()
    assert np.array_equal(bits(tr.cpu().numpy()), bits(r)) and np.array_equal(tg.cpu().numpy(), g) and np.array_equal(bits(tp.cpu().numpy()), bits(pts))
    assert np.array_equal(bits(t2.cpu().numpy()), bits(r)), "without the geom-id and point images the range bits are the same"
    only_r = np.full((n, height, width), 7.0, dtype=np.float32)
    o, table = e._scan_options(1, width, height, (pattern[2], pattern[3]), pattern[4], dict(bodyexclude=bd))
    assert e.lib.mjh_scan(e.h, env0, n, C.byref(o), C.c_void_p(only_r.ctypes.data), None, None) == 0
    assert np.array_equal(bits(only_r), bits(r))


# ------------------------------------------------------------------ 5. more geoms than one staging pass holds; meshes; a height field
def test_more_geoms_than_one_staging_pass(lib):
    m = spheres_model(lib)
    assert m.ngeom == 72
    e = ms.Engine(m, NENV)
    r, g = scan(e, "lidar", SPHERES_PATTERN)
    for env in range(1, NENV):
        assert np.array_equal(bits(r[env]), bits(r[0])) and np.array_equal(g[env], g[0])
    check("71 spheres", r[0], g[0], device_scene(e, m, 0), sensor_rays(e, m, 0, 0, SPHERES_PATTERN))
    assert (g[0] >= 64).any() and ((g[0] > 0) & (g[0] < 64)).any(), "geoms of both staging passes are seen"
    e.close()


@pytest.mark.parametrize("ngeom", [65, 130])
def test_staging_pass_edges(lib, ngeom):
    """65 geoms: the second staging pass holds a single candidate; 130: a third pass follows a full second one.  The sensor hangs over
    the last sphere and looks down; 5 rows of 9 beams: tiles partial in both directions"""
    spec, last = rr.pass_edge_spec(ngeom)
    pattern = (9, 5, -np.pi, 2 * np.pi / 9, (-85.0 * DEG, 9.0 * DEG))
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, spec)
    add_site(lib, b, b"lidar", 0, ((last[0] - 0.2, last[1] - 0.1, 1.7), yaw(0.3)))
    m = compile_model(lib, b)
    assert m.ngeom == ngeom
    e = ms.Engine(m, NENV)
    r, g = scan(e, "lidar", pattern)      # (cull 0 and cull 1: the same bits)
    for env in range(1, NENV):
        assert np.array_equal(bits(r[env]), bits(r[0])) and np.array_equal(g[env], g[0])
    check(f"{ngeom} geoms 5x9", r[0], g[0], device_scene(e, m, 0), sensor_rays(e, m, 0, 0, pattern))
    assert (g[0] == ngeom - 1).any(), "the last geom, in the last pass, is seen"
    assert all(((g[0] >= 64 * p) & (g[0] < 64 * (p + 1))).any() for p in range((ngeom + 63) // 64)), "geoms of every staging pass are seen"
    e.close()


def test_tetrahedron_field_in_mesh_mode_1(lib):
    m = tetra_model(lib)
    assert m.ngeom == 107 and (m.array("geom_type") == rr.MESH).sum() == 70
    e = ms.Engine(m, NENV)
    e.ray_mesh_mode = 1
    tris = [rm.hull_triangles(x) for x in rm.model_mesh_verts(m)]
    r, g = scan(e, "lidar", TETRA_PATTERN)
    for env in range(1, NENV):
        assert np.array_equal(bits(r[env]), bits(r[0])) and np.array_equal(g[env], g[0])
    check("tetrahedron field", r[0], g[0], device_scene(e, m, 0, tris=tris), sensor_rays(e, m, 0, 0, TETRA_PATTERN))
    types = m.array("geom_type")
    assert len({int(x) for x in g[0].ravel() if x >= 0 and types[x] == rr.MESH}) >= 10, "at least ten different mesh geoms are seen"
    assert (g[0] >= 64).any() and ((g[0] > 0) & (g[0] < 64)).any()
    e.close()


def test_mesh_surface_1(lib):
    m = tri_model(lib)
    e = ms.Engine(m, NENV)
    e.ray_mesh_mode = 1; e.ray_mesh_surface = 1
    tris = rt.model_mesh_tris(m)
    r, g = scan(e, "scanner", TRI_PATTERN)
    check("mesh surface 1", r[0], g[0], device_scene(e, m, 0, tris=tris), sensor_rays(e, m, 0, 0, TRI_PATTERN))
    mesh = np.nonzero(m.array("geom_type") == rr.MESH)[0]
    assert all((g[0] == k).sum() >= 4 for k in mesh), "every mesh is seen"
    e.ray_mesh_surface = 0
    rh, gh = scan(e, "scanner", TRI_PATTERN, n=1)
    assert not np.array_equal(rh[0], r[0]), "the hull of the torus and of the jaw is another surface"
    e.close()


def test_hfield(lib):
    import hfield_ref
    m = hfield_model(lib)
    e = ms.Engine(m, NENV)
    r, g = scan(e, "lidar", HFIELD_PATTERN)
    scene = device_scene(e, m, 0, hfield={0: hfield_ref.hfield_of(m, 0)})
    rays = sensor_rays(e, m, 0, 0, HFIELD_PATTERN)
    for env in range(NENV):
        check(f"hfield env {env}", r[env], g[env], scene, rays)
    assert (g[0] == 0).mean() > 0.3
    e.close()


# ------------------------------------------------------------------ 6. options
def test_cutoff(prim):
    m, e, scene = prim
    pattern = sr.PATTERNS["full turn 16x360"]
    rays = sensor_rays(e, m, 0, 0, pattern)
    r0, g0 = scan(e, "lidar", pattern, n=1)
    ref_d, ref_g = rm.cast(rays[0], rays[1], scene)
    cut = 0.5 * (ref_d[ref_g >= 0].min() + ref_d[ref_g >= 0].max())
    rc, gc = scan(e, "lidar", pattern, n=1, cutoff=cut)
    check("cutoff", rc[0], gc[0], scene, rays, cutoff=cut)
    far = r0[0] > np.float32(cut)
    assert far.any() and (g0[0][~far] >= 0).any()
    assert (rc[0][far] == -1.0).all() and (gc[0][far] == -1).all()
    assert np.array_equal(bits(rc[0][~far]), bits(r0[0][~far])) and np.array_equal(gc[0][~far], g0[0][~far]), "the rest is unchanged"
    _, _, pts = e.scan("lidar", **sr.scan_kwargs(pattern), n=1, cutoff=cut, points=True)
    assert (pts[0][far] == 0.0).all(), "a beam beyond the cutoff is a miss in the point cloud too"


def test_flg_static(prim):
    m, e, scene = prim
    pattern = sr.PATTERNS["full turn 16x360"]
    body = m.array("geom_bodyid")
    r, g = scan(e, "lidar", pattern, n=1, flg_static=0)
    check("flg_static 0", r[0], g[0], dict(scene, visible=body != 0), sensor_rays(e, m, 0, 0, pattern))
    assert (body[g[0][g[0] >= 0]] != 0).all() and (g[0] >= 0).any()


def test_inactive_slot_hides_its_body_in_that_env_only(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    pattern = sr.PATTERNS["full turn 16x360"]
    body = m.array("geom_bodyid")
    r0, g0 = scan(e, "lidar", pattern)
    seen = [int(g) for g in np.unique(g0[0]) if g >= 0 and body[g] > 0]
    g = max(seen, key=lambda k: int((g0[0] == k).sum())); bd = int(body[g])
    e.set_slot_active(bd, 0, env0=2, n=1)
    r1, g1 = scan(e, "lidar", pattern)
    assert not (g1[2] == g).any() and (g1[0] == g).any()
    for env in (0, 1, 3):
        assert np.array_equal(r1[env], r0[env]) and np.array_equal(g1[env], g0[env])
    check("inactive slot", r1[2], g1[2], device_scene(e, m, 2, visible=body != bd), sensor_rays(e, m, 0, 2, pattern))
    e.set_slot_active(bd, 1, env0=2, n=1)
    r2, g2 = e.scan("lidar", **sr.scan_kwargs(pattern))
    assert np.array_equal(r2, r0) and np.array_equal(g2, g0)
    e.close()


# ------------------------------------------------------------------ 7. nothing of the state is written
def _snapshot(e):
    t, q, v, w = e.get_state()
    return [t, q, v, w, e.get_stats(), e.get_field("qacc"), e.get_field("qfrc_applied")]


def test_no_side_effects(lib):
    m = prim_model(lib, gravity=(0, 0, -9.81))
    a, b = ms.Engine(m, NENV), ms.Engine(m, NENV)
    a.step(150); b.step(150)      # (the free bodies have begun to land on the floor)
    before = _snapshot(a)
    a.scan("lidar", **sr.scan_kwargs(sr.PATTERNS["9x70"])); a.scan("lidar", **sr.scan_kwargs(sr.PATTERNS["table 9x70"]), env0=1, n=2, cull=0, points=True)
    for x, y in zip(before, _snapshot(a)):
        assert np.array_equal(x, y)
    a.step(3); b.step(3)
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "a step after a scan equals a step without one"
    # ... and between the halves of a split step, as mjh_ray
    a.step1(); r, g = a.scan("lidar", **sr.scan_kwargs(sr.PATTERNS["9x70"])); a.step2()
    b.step1(); b.get_geom_state(0, NENV); b.step2()
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "the call sequence rules are those of mjh_get_geom_state"
    assert (g >= 0).any()
    a.close(); b.close()


def test_a_pattern_is_uploaded_when_it_changes(prim):
    """the tables follow the pattern: alternating patterns of the same size give what each gives alone"""
    m, e, scene = prim
    pa = sr.PATTERNS["9x70"]
    pb = (pa[0], pa[1], pa[2] + 0.5, pa[3], pa[4]); pc = (pa[0], pa[1], pa[2], pa[3], sr.TABLE9); pd = (pa[0], pa[1], pa[2], pa[3], sr.TABLE9[::-1].copy())
    first = [e.scan("lidar", **sr.scan_kwargs(p), n=1) for p in (pa, pb, pc, pd)]
    assert not np.array_equal(first[0][0], first[1][0]) and not np.array_equal(first[2][0], first[3][0])
    assert np.array_equal(bits(first[2][0][0]), bits(first[3][0][0][::-1])), "the reversed table gives the rows in reverse"
    for p, (r, g) in list(zip((pa, pb, pc, pd), first))[::-1]:
        r2, g2 = e.scan("lidar", **sr.scan_kwargs(p), n=1)
        assert np.array_equal(bits(r2), bits(r)) and np.array_equal(g2, g)


# ------------------------------------------------------------------ 8. errors
def test_errors_launch_nothing(prim, lib):
    m, e, scene = prim
    width, height = 9, 3
    kw = dict(width=width, height=height, azimuth=(-0.5, 0.1), elevation=(-0.3, 0.2))
    good_r, good_g, good_p = e.scan("lidar", points=True, **kw)
    rng_ = np.full((NENV, height, width), 7.0, dtype=np.float32); gid = np.full((NENV, height, width), 7, dtype=np.int32)
    pts = np.full((NENV, height, width, 3), 7.0, dtype=np.float32)
    bad_table = np.array([0.0, 1.6, 0.1]); nan_table = np.array([0.0, np.nan, 0.1])

    def call(eng=e, env0=0, n=NENV, null=False, table=None, **opt):
        o = capi.ScanOptions(); lib.mjh_scan_default_options(C.byref(o))
        o.site, o.width, o.height, o.azimuth0, o.azimuth_step, o.elevation0, o.elevation_step = 0, width, height, -0.5, 0.1, -0.3, 0.2
        if table is not None:
            o.elevation = capi.dptr(table)
        for k, v in opt.items():
            setattr(o, k, v)
        return lib.mjh_scan(eng.h, env0, n, C.byref(o), None if null else C.c_void_p(rng_.ctypes.data), C.c_void_p(gid.ctypes.data), C.c_void_p(pts.ctypes.data))

    def ok():
        assert (rng_ == 7.0).all() and (gid == 7).all() and (pts == 7.0).all(), "nothing was launched: the outputs are untouched"
        assert call() == 0
        assert np.array_equal(rng_, good_r) and np.array_equal(gid, good_g) and np.array_equal(pts, good_p)
        rng_[:] = 7.0; gid[:] = 7; pts[:] = 7.0

    for bad in (dict(site=1), dict(site=-2), dict(bodyexclude=m.nbody), dict(bodyexclude=-2), dict(width=0), dict(height=0), dict(width=-3),
                dict(width=1 << 16, height=1 << 15, elevation_step=0.0), dict(azimuth0=np.nan), dict(azimuth_step=np.inf), dict(elevation0=np.nan),
                dict(elevation_step=-np.inf), dict(elevation0=-1.7), dict(elevation_step=1.0), dict(table=bad_table), dict(table=nan_table),
                dict(env0=2, n=3), dict(env0=-1, n=2), dict(env0=NENV, n=1), dict(n=0), dict(null=True)):
        assert call(**bad) == MJH_ERR_ARG, bad
        assert lib.mjh_last_error()
        ok()
    assert lib.mjh_scan_device(e.h, 0, NENV, None, None, None, None) == MJH_ERR_ARG
    ok()
    with pytest.raises(MjhError):
        e.scan("lidar", 0, 8)
    with pytest.raises(ValueError):
        e.scan("no such site", 8, 8)
    with pytest.raises(ValueError):
        e.scan("lidar", 8, 3, elevation=np.zeros(4))
    with pytest.raises(TypeError):
        e.scan("lidar", 8, 8, per_env=1)
    ok()
