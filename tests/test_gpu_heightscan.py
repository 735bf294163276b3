"""Height scans on the device (mjh_heightscan / mjh_heightscan_device, csrc/heightscan.hip) against the fp64 references ray_ref.cast /
ray_mesh_ref.cast.

The reference casts rays generated in numpy fp64 (tests/heightscan_ref.py: the grid frame of the alignment, the cell coordinates) at
the device's own site pose: the site body's pose (mjh_get_body_state) composed with the model's site_pos / site_quat, and against the
geom poses of mjh_get_geom_state.  Only the scan arithmetic is under test.  The rule is ray_check.check's, the project's: on the rays
robust() accepts the geom ids are equal, misses are exactly -1 and |range - ref| <= 5e-5 max(1, ref); at most 2 % of a scan's rays
may be non-robust.  The sensors and grids stand where the reference alone finds at most 1 % of the rays non-robust (computed on the
CPU from the models' initial poses before anything ran on a GPU; the share of every case is printed).  Every scan is cast with
cull = 1 and cull = 0 and the two must be the same bits (the contract of the tile cull).

Measured on one MI355X (`pytest tests/test_gpu_heightscan.py -m gpu -s` prints every case), max scaled error / non-robust share:
primitives 41 x 23 1.0e-06 / 0.21 %, 130 x 1 2.3e-07 / 0.77 %, 9 x 70 5.5e-07 / 0.32 %, 5 x 3 1.6e-07 / 0, 1 x 1 1.9e-08 / 0 (each the
worst of the three alignments), the default struct 1.9e-07 / 0.39 %, world frame 3.0e-07 / 0; sensor on a free body, four poses x
three alignments: own body hidden 6.6e-07 / 0.42 %, from inside its ball 3.1e-07 / 0; exclude_tree: bodyexclude alone 1.6e-07 /
0.31 %, the tree 7.6e-08 / 0; rotated height field 3.5e-07 / 0.97 %, terrain C at its nodes 7.4e-08 / 0; 71 spheres 7.9e-07 / 0.21 %;
tetrahedron field (mesh mode 1) 3.6e-07 / 0.10 %; mesh surface 1 4.5e-07 / 0; cutoff 1.0e-06, flg_static 1.7e-07, inactive slot
1.7e-07 / at most 0.21 %; points within 1.5e-07 of (x_j, y_i, above - range); against mjh_ray fed the same rays 6.5e-07, 43 - 49 % of
the ranges bitwise equal.  Worst over all cases 1.0e-06 (bound 5e-05), largest non-robust share 0.97 % (cap 2 %)."""
import ctypes as C

import numpy as np
import pytest

import heightscan_ref as hr
import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr
import ray_tri_ref as rt
from helpers import D, set_opt
from mujoco_sim_amd import capi
from mujoco_sim_amd.engine import MjhError
from ray_check import TOL, check
# the lidar tests' model helpers and their mesh scene serve here unchanged
from test_gpu_scan import TRI_ITEMS, _snapshot, add_site, add_spec, bits, compile_model, device_scene, far_body, unit, yaw

pytestmark = pytest.mark.gpu

MJH_ERR_ARG = -1
NENV = 4


# the sensors: (site_pos, site_quat) in their body
PRIM_SENSOR = ((0.1, 0.05, 2.2), unit((0.98, 0.05, -0.08, 0.15)))      # above the primitives, rolled, pitched and yawed
RIG_SENSOR = ((0.03, 0.01, 0.02), (1.0, 0.0, 0.0, 0.0))                  # inside the rig's ball, in the body's own orientation
RIG_RADIUS = 0.12
RIG_GRID = (24, 20, (0.1, 0.08), (0.1, 0.0), 0.5)
INSIDE_GRID = (5, 3, (0.02, 0.02), (0.0, 0.0), 0.05)                     # every start point lies inside the ball
HFIELD_SENSOR = ((0.3, -0.2, 1.3), yaw(1.1))
HFIELD_GRID = (48, 30, (0.05, 0.05), (0.0, 0.0), 0.4)
SPHERES_SENSOR = ((0.0, 0.225, 2.4), yaw(0.3))
SPHERES_GRID = (40, 24, (0.1, 0.1), (0.0, 0.0), 0.5)
TETRA_SENSOR = ((0.0, 0.225, 2.4), yaw(-0.7))
TETRA_GRID = (40, 24, (0.1, 0.1), (0.0, 0.0), 0.5)
TRI_SENSOR = ((0.0, 0.1, 2.0), yaw(0.4))
TRI_GRID = (44, 40, (0.06, 0.06), (0.0, 0.0), 0.5)
TREE_GRID = (20, 16, (0.08, 0.08), (0.0, 0.0), 0.5)
WORLD_GRID = (32, 12, (0.17, 0.3), (0.0, 0.4), 3.0)


# ------------------------------------------------------------------ the sensor's rays in fp64
def site_pose(e, m, site, env):
    """(o, S) of site `site` in env `env` from the device's own body pose; site None: the world frame"""
    if site is None:
        return np.zeros(3), np.eye(3)
    xp, xq = e.get_body_state(env, 1)
    b = int(m.array("site_bodyid")[site])
    Rb = rr.quat2mat(xq[0, b]).reshape(3, 3)
    return xp[0, b] + Rb @ m.array("site_pos").reshape(-1, 3)[site], Rb @ rr.quat2mat(m.array("site_quat").reshape(-1, 4)[site]).reshape(3, 3)


def sensor_rays(e, m, site, env, grid, align):
    return hr.rays64(site_pose(e, m, site, env), grid, align)


def hscan(e, site, grid, align="yaw", **kw):
    """the scan with the cull on, after checking that the cull off gives the same bits"""
    r1, g1 = e.height_scan(site, **hr.kwargs(grid), align=align, cull=1, **kw)
    r0, g0 = e.height_scan(site, **hr.kwargs(grid), align=align, cull=0, **kw)
    assert r1.dtype == np.float32 and g1.dtype == np.int32 and r1.shape == g1.shape == (kw.get("n") or e.nenv - kw.get("env0", 0), grid[1], grid[0])
    assert np.array_equal(bits(r1), bits(r0)) and np.array_equal(g1, g0), "cull = 1 and cull = 0 give the same bits"
    return r1, g1


# ------------------------------------------------------------------ models
def prim_model(lib, gravity=(0, 0, 0), rig=False):
    """ray_ref.primitives_spec() with the sensor `scanner` on the world body above them; rig: one more free body (a ball) that carries
    the sensor `head` inside its own geom"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=list(gravity))
    add_spec(lib, b, rr.primitives_spec())
    add_site(lib, b, b"scanner", 0, PRIM_SENSOR)
    if rig:
        bd = lib.mjh_builder_add_body(b, b"rig", 0, D(0.0, 0.0, 2.2), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_geom(b, b"rigg", bd, rr.SPHERE, D(RIG_RADIUS, 0, 0), None, None, None, -1, -1, -1, -1) >= 0
        assert add_site(lib, b, b"head", bd, RIG_SENSOR) == 1
    return compile_model(lib, b)


RIG_POSES = [((-0.4, 0.1, 2.2), unit((0.97, 0.1, -0.12, 0.2))), ((0.5, -0.2, 2.4), unit((0.8, -0.15, 0.1, -0.55))),
             ((0.1, 0.3, 2.0), unit((0.35, 0.08, 0.05, 0.93))), ((-0.2, -0.1, 2.3), (np.sqrt(0.5), 0.0, np.sqrt(0.5), 0.0))]      # the last: pitched exactly 90 degrees


def rig_qpos(m):
    bd = m.name2id(0, "rig")
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[bd]])
    q = np.tile(m.array("qpos0"), (NENV, 1))
    for i, (pos, quat) in enumerate(RIG_POSES):
        q[i, adr:adr + 3] = pos; q[i, adr + 3:adr + 7] = quat
    return q


def tree_model(lib):
    """a floor, a base (free body, a ball around the sensor `head`) that carries an arm on a hinge with a box under the grid, and another
    free body, a sphere, under the grid too"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=[0, 0, 0])
    assert lib.mjh_builder_add_geom(b, b"floor", 0, rr.PLANE, D(3.0, 3.0, 0.05), D(0, 0, 0), None, None, -1, -1, -1, -1) >= 0
    base = lib.mjh_builder_add_body(b, b"base", 0, D(0.0, 0.0, 1.5), D(*yaw(0.5)), 0.0)
    lib.mjh_builder_add_joint(b, None, base, 0, None, None, None, 0, 0, 0, 0, 0)
    assert lib.mjh_builder_add_geom(b, b"baseg", base, rr.SPHERE, D(0.1, 0, 0), None, None, None, -1, -1, -1, -1) >= 0
    arm = lib.mjh_builder_add_body(b, b"arm", base, D(0.3, 0.1, -0.4), None, 0.0)
    lib.mjh_builder_add_joint(b, b"elbow", arm, 3, None, D(0, 1, 0), None, 0, 0, 0, 0, 0)
    assert lib.mjh_builder_add_geom(b, b"armg", arm, rr.BOX, D(0.2, 0.15, 0.05), D(0.1, 0.0, -0.1), D(*unit((0.95, 0.05, 0.08, 0.29))), None, -1, -1, -1, -1) >= 0
    other = lib.mjh_builder_add_body(b, b"other", 0, D(-0.43, -0.17, 0.6), None, 0.0)
    lib.mjh_builder_add_joint(b, None, other, 0, None, None, None, 0, 0, 0, 0, 0)
    assert lib.mjh_builder_add_geom(b, b"otherg", other, rr.SPHERE, D(0.21, 0, 0), None, None, None, -1, -1, -1, -1) >= 0
    add_site(lib, b, b"head", base, ((0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0)))
    return compile_model(lib, b)


def spheres_model(lib):
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, rr.many_spheres_spec())
    far_body(lib, b)
    add_site(lib, b, b"scanner", 0, SPHERES_SENSOR)
    return compile_model(lib, b)


def tetra_model(lib):
    """ray_mesh_ref.tetra_field_spec(): 70 tetrahedron-mesh geoms of one asset and 35 spheres over a floor, the sensor above them"""
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
    add_site(lib, b, b"scanner", 0, TETRA_SENSOR)
    return compile_model(lib, b)


def hfield_model(lib, hf, pos, quat, sensor):
    nrow, ncol, size, elev = hf
    b = lib.mjh_builder_create()
    el = (C.c_double * elev.size)(*elev.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", nrow, ncol, D(*size), el)
    assert h >= 0
    assert lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*pos), D(*quat), None, -1, -1, -1) >= 0
    far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    add_site(lib, b, b"scanner", 0, sensor)
    return compile_model(lib, b)


@pytest.fixture(scope="module")
def prim(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    yield m, e, device_scene(e, m, 0)
    e.close()


# ------------------------------------------------------------------ 1. every primitive type under the sensor, every grid and alignment
@pytest.mark.parametrize("align", hr.ALIGNS)
@pytest.mark.parametrize("name", list(hr.GRIDS))
def test_primitives(prim, lib, name, align):
    m, e, scene = prim
    grid = hr.GRIDS[name]
    rng_, gid = hscan(e, "scanner", grid, align)
    for env in range(1, NENV):      # no per-env data: every env sees the same scene
        assert np.array_equal(bits(rng_[env]), bits(rng_[0])) and np.array_equal(gid[env], gid[0])
    check(f"primitives {name} {align}", rng_[0], gid[0], scene, sensor_rays(e, m, 0, 0, grid, align))
    r2, g2 = e.height_scan(0, **hr.kwargs(grid), align=align)      # by id, the default options
    assert np.array_equal(bits(r2), bits(rng_)) and np.array_equal(g2, gid)
    if name == "41x23":
        assert {int(scene["type"][g]) for g in gid[0].ravel() if g >= 0} >= {rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.ELLIPSOID, rr.CYLINDER, rr.BOX}


def test_default_options(prim, lib):
    m, e, scene = prim
    o = capi.HeightScanOptions(); lib.mjh_heightscan_default_options(C.byref(o))
    assert (o.site, o.align, o.width, o.height, o.bodyexclude, o.exclude_tree, o.flg_static, o.cull, o.cutoff) == (-1, 0, 16, 16, -1, 0, 1, 1, 0.0)
    assert tuple(o.spacing) == (0.1, 0.1) and tuple(o.offset) == (0.0, 0.0) and o.above == 1.0
    o.site = 0
    r = np.zeros((NENV, 16, 16), dtype=np.float32); g = np.zeros((NENV, 16, 16), dtype=np.int32)
    assert lib.mjh_heightscan(e.h, 0, NENV, C.byref(o), C.c_void_p(r.ctypes.data), C.c_void_p(g.ctypes.data), None) == 0
    r2, g2 = e.height_scan("scanner", 16, 16, 0.1)
    assert np.array_equal(bits(r), bits(r2)) and np.array_equal(g, g2)
    check("default struct", r[0], g[0], scene, sensor_rays(e, m, 0, 0, (16, 16, (0.1, 0.1), (0.0, 0.0), 1.0), "yaw"))


# ------------------------------------------------------------------ 2. the world frame
@pytest.mark.parametrize("align", hr.ALIGNS)
def test_world_frame(prim, align):
    """site None is the world frame: the three alignments are one grid, cast from 3 m above the floor's origin"""
    m, e, scene = prim
    r, g = hscan(e, None, WORLD_GRID, align, n=1)
    check(f"world frame {align}", r[0], g[0], scene, sensor_rays(e, m, None, 0, WORLD_GRID, align))
    rw, gw = e.height_scan(-1, **hr.kwargs(WORLD_GRID), align="world", n=1)
    assert np.array_equal(bits(r), bits(rw)) and np.array_equal(g, gw)
    assert (g[0] > 0).sum() >= 20 and (g[0] == 0).sum() >= 20


# ------------------------------------------------------------------ 3. a sensor on a free body, its own pose in every env
@pytest.fixture(scope="module")
def rig(lib):
    m = prim_model(lib, rig=True)
    e = ms.Engine(m, NENV)
    e.set_state(qpos=rig_qpos(m), qvel=np.zeros((NENV, m.nv)))
    e.forward()
    yield m, e, m.name2id(0, "rig")
    e.close()


@pytest.mark.parametrize("align", hr.ALIGNS)
def test_sensor_on_a_free_body(rig, align):
    m, e, bd = rig
    body = m.array("geom_bodyid")
    rigg = int(np.nonzero(body == bd)[0][0])
    r, g = hscan(e, "head", RIG_GRID, align, bodyexclude=bd)
    ri, gi = hscan(e, "head", INSIDE_GRID, align)
    xp, _ = e.get_body_state()
    assert np.abs(xp[0, bd] - xp[1, bd]).max() > 0.1, "every env has its own sensor pose"
    for env in range(NENV):
        check(f"rig {align} env {env} (own body hidden)", r[env], g[env], device_scene(e, m, env, visible=body != bd), sensor_rays(e, m, 1, env, RIG_GRID, align))
        assert not (g[env] == rigg).any()
        # the grid starts inside its body's ball: every ray sees the ball's far surface
        check(f"rig {align} env {env} (from inside)", ri[env], gi[env], device_scene(e, m, env), sensor_rays(e, m, 1, env, INSIDE_GRID, align))
        assert (gi[env] == rigg).all() and ri[env].max() < 2 * RIG_RADIUS
    assert not np.array_equal(r[0], r[1])
    # env 3 is pitched exactly 90 degrees: the site's x axis is vertical and the YAW grid takes the world's x axis
    o, S = site_pose(e, m, 1, 3)
    assert S[0, 0] ** 2 + S[1, 0] ** 2 < hr.DEGENERATE and abs(S[2, 0]) > 0.999
    if align == "yaw":
        assert np.array_equal(hr.grid_frame(S, "yaw"), np.eye(3))
        assert (g[3] >= 0).mean() > 0.5, "the fallen-back grid still looks down at the scene"
    if align == "base":
        assert (g[:3] >= 0).mean() > 0.3


# ------------------------------------------------------------------ 4. exclude_tree
def test_exclude_tree(lib):
    m = tree_model(lib)
    e = ms.Engine(m, NENV)
    base, arm, other = (m.name2id(0, n) for n in ("base", "arm", "other"))
    root = m.array("body_rootid")
    assert root[arm] == base and root[base] == base and root[other] == other
    q = np.tile(m.array("qpos0"), (NENV, 1))
    adr = int(m.array("jnt_qposadr")[m.name2id(1, "elbow")])
    q[:, adr] = [0.0, 0.3, -0.4, 0.7]      # the arm at another angle in every env
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv))); e.forward()
    body = m.array("geom_bodyid")
    armg, otherg, baseg = (m.name2id(2, n) for n in ("armg", "otherg", "baseg"))
    for align in hr.ALIGNS:
        r1, g1 = hscan(e, "head", TREE_GRID, align, bodyexclude=base)
        rt_, gt = hscan(e, "head", TREE_GRID, align, bodyexclude=base, exclude_tree=1)
        ra, ga = hscan(e, "head", TREE_GRID, align, bodyexclude=arm, exclude_tree=1)      # any body of the tree names it
        assert np.array_equal(bits(ra), bits(rt_)) and np.array_equal(ga, gt)
        for env in range(NENV):
            rays = sensor_rays(e, m, 0, env, TREE_GRID, align)
            check(f"tree {align} env {env} (bodyexclude alone)", r1[env], g1[env], device_scene(e, m, env, visible=body != base), rays)
            check(f"tree {align} env {env} (exclude_tree)", rt_[env], gt[env], device_scene(e, m, env, visible=root[body] != base), rays)
            assert (g1[env] == armg).any() and not (g1[env] == baseg).any(), "with bodyexclude alone the arm's box is seen"
            assert not (gt[env] == armg).any() and not (gt[env] == baseg).any(), "with exclude_tree the whole tree is hidden"
            assert (gt[env] == otherg).any() and (gt[env] == 0).any(), "the other body and the floor are still seen"
    r0, g0 = hscan(e, "head", TREE_GRID, "yaw")
    assert (g0 == baseg).any(), "without bodyexclude the base is seen from above"
    e.close()


# ------------------------------------------------------------------ 5. height fields
def test_rotated_hfield(lib):
    m = hfield_model(lib, (rr.HF_NROW, rr.HF_NCOL, np.array(rr.HF_SIZE), rr.HF_ELEV), rr.HF_POS, rr.HF_QUAT, HFIELD_SENSOR)
    import hfield_ref
    e = ms.Engine(m, NENV)
    scene = device_scene(e, m, 0, hfield={0: hfield_ref.hfield_of(m, 0)})
    for align in hr.ALIGNS:
        r, g = hscan(e, "scanner", HFIELD_GRID, align)
        for env in range(NENV):
            check(f"rotated hfield {align} env {env}", r[env], g[env], scene, sensor_rays(e, m, 0, 0, HFIELD_GRID, align))
        hits = int((g[0] == 0).sum())
        assert 700 <= hits <= 1100, "misses beyond the field's edges are exercised"
    e.close()


def test_terrain_heights_at_the_nodes(lib):
    """the unrotated terrain C under a WORLD grid laid exactly on its inner nodes: the range is the start height minus the node's height"""
    hf = rr.terrain("C")
    nrow, ncol, size, elev = hf
    assert (nrow, ncol) == (17, 33)
    dx, dy = 2 * size[0] / (ncol - 1), 2 * size[1] / (nrow - 1)
    m = hfield_model(lib, hf, (0.0, 0.0, 0.0), (1.0, 0.0, 0.0, 0.0), ((0.0, 0.0, 2.0), yaw(0.8)))
    e = ms.Engine(m, NENV)
    grid = (ncol - 2, nrow - 2, (dx, dy), (0.0, 0.0), 0.5)
    assert grid[:2] == (31, 15)
    r, g = hscan(e, "scanner", grid, "world")
    assert (g == 0).all(), "every ray hits"
    expect = 2.5 - elev[1:-1, 1:-1] * size[2]      # (row r of the field is y = -size_y + r dy, column c is x = -size_x + c dx: the grid's own order)
    err = np.abs(r.astype(float) - expect[None]) / np.maximum(1.0, expect[None])
    print(f"terrain C at the nodes: max scaled error {err.max():.3e}")
    assert err.max() <= TOL
    import hfield_ref
    check("terrain C", r[0], g[0], device_scene(e, m, 0, hfield={0: hfield_ref.hfield_of(m, 0)}), sensor_rays(e, m, 0, 0, grid, "world"))
    e.close()


# ------------------------------------------------------------------ 6. more geoms than one staging pass holds; 7. mesh surface 1
def test_more_geoms_than_one_staging_pass(lib):
    m = spheres_model(lib)
    assert m.ngeom == 72
    e = ms.Engine(m, NENV)
    for align in ("yaw", "base"):
        r, g = hscan(e, "scanner", SPHERES_GRID, align)
        for env in range(1, NENV):
            assert np.array_equal(bits(r[env]), bits(r[0])) and np.array_equal(g[env], g[0])
        check(f"71 spheres {align}", r[0], g[0], device_scene(e, m, 0), sensor_rays(e, m, 0, 0, SPHERES_GRID, align))
        assert (g[0] >= 64).any() and ((g[0] > 0) & (g[0] < 64)).any(), "geoms of both staging passes are seen"
    e.close()


@pytest.mark.parametrize("ngeom", [65, 130])
def test_staging_pass_edges(lib, ngeom):
    """65 geoms: the second staging pass holds a single candidate; 130: a third pass follows a full second one.  The sensor hangs over
    the last sphere; 5 rows of 9 cells: tiles partial in both directions"""
    spec, last = rr.pass_edge_spec(ngeom)
    grid = (9, 5, (0.12, 0.11), (0.0, 0.0), 0.5)
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    add_spec(lib, b, spec)
    add_site(lib, b, b"scanner", 0, ((last[0] - 0.2, last[1] - 0.1, 2.4), yaw(0.3)))
    m = compile_model(lib, b)
    assert m.ngeom == ngeom
    e = ms.Engine(m, NENV)
    for align in ("yaw", "base"):
        r, g = hscan(e, "scanner", grid, align)      # (cull 0 and cull 1: the same bits)
        for env in range(1, NENV):
            assert np.array_equal(bits(r[env]), bits(r[0])) and np.array_equal(g[env], g[0])
        check(f"{ngeom} geoms 5x9 {align}", r[0], g[0], device_scene(e, m, 0), sensor_rays(e, m, 0, 0, grid, align))
        assert (g[0] == ngeom - 1).any(), "the last geom, in the last pass, is seen"
        assert all(((g[0] >= 64 * p) & (g[0] < 64 * (p + 1))).any() for p in range((ngeom + 63) // 64)), "geoms of every staging pass are seen"
    e.close()


def test_tetrahedron_field_in_mesh_mode_1(lib):
    m = tetra_model(lib)
    assert m.ngeom == 107 and (m.array("geom_type") == rr.MESH).sum() == 70
    e = ms.Engine(m, NENV)
    e.ray_mesh_mode = 1
    tris = [rm.hull_triangles(x) for x in rm.model_mesh_verts(m)]
    r, g = hscan(e, "scanner", TETRA_GRID)
    for env in range(1, NENV):
        assert np.array_equal(bits(r[env]), bits(r[0])) and np.array_equal(g[env], g[0])
    check("tetrahedron field", r[0], g[0], device_scene(e, m, 0, tris=tris), sensor_rays(e, m, 0, 0, TETRA_GRID, "yaw"))
    types = m.array("geom_type")
    assert len({int(x) for x in g[0].ravel() if x >= 0 and types[x] == rr.MESH}) >= 10, "at least ten different mesh geoms are seen"
    assert (g[0] >= 64).any() and ((g[0] > 0) & (g[0] < 64)).any()
    e.close()


def test_mesh_surface_1(lib):
    m = rt.scene_model(lib, TRI_ITEMS, site=(0, *TRI_SENSOR))[0]
    e = ms.Engine(m, NENV)
    e.ray_mesh_mode = 1; e.ray_mesh_surface = 1
    tris = rt.model_mesh_tris(m)
    r, g = hscan(e, "scanner", TRI_GRID)
    check("mesh surface 1", r[0], g[0], device_scene(e, m, 0, tris=tris), sensor_rays(e, m, 0, 0, TRI_GRID, "yaw"))
    mesh = np.nonzero(m.array("geom_type") == rr.MESH)[0]
    assert all((g[0] == k).sum() >= 4 for k in mesh), "every mesh is seen"
    e.ray_mesh_surface = 0
    rh, gh = hscan(e, "scanner", TRI_GRID, n=1)
    assert not np.array_equal(rh[0], r[0]), "the hull of the torus and of the jaw is another surface"
    e.close()


# ------------------------------------------------------------------ 8. options
def test_cutoff(prim):
    m, e, scene = prim
    grid = hr.GRIDS["41x23"]
    rays = sensor_rays(e, m, 0, 0, grid, "base")
    r0, g0 = hscan(e, "scanner", grid, "base", n=1)
    ref_d, ref_g = rm.cast(rays[0], rays[1], scene)
    cut = 0.5 * (ref_d[ref_g >= 0].min() + ref_d[ref_g >= 0].max())
    rc, gc = hscan(e, "scanner", grid, "base", n=1, cutoff=cut)
    check("cutoff", rc[0], gc[0], scene, rays, cutoff=cut)
    far = r0[0] > np.float32(cut)
    assert far.any() and (g0[0][~far] >= 0).any()
    assert (rc[0][far] == -1.0).all() and (gc[0][far] == -1).all()
    assert np.array_equal(bits(rc[0][~far]), bits(r0[0][~far])) and np.array_equal(gc[0][~far], g0[0][~far]), "the rest is unchanged"
    _, _, pts = e.height_scan("scanner", **hr.kwargs(grid), align="base", n=1, cutoff=cut, points=True)
    assert (pts[0][far][:, 2] == np.float32(grid[4])).all(), "a ray beyond the cutoff is a miss in the points too: its start"


def test_flg_static(prim):
    m, e, scene = prim
    grid = hr.GRIDS["41x23"]
    body = m.array("geom_bodyid")
    r, g = hscan(e, "scanner", grid, n=1, flg_static=0)
    check("flg_static 0", r[0], g[0], dict(scene, visible=body != 0), sensor_rays(e, m, 0, 0, grid, "yaw"))
    assert (body[g[0][g[0] >= 0]] != 0).all() and (g[0] >= 0).any() and (g[0] < 0).any()


def test_inactive_slot_hides_its_body_in_that_env_only(lib):
    m = prim_model(lib)
    e = ms.Engine(m, NENV)
    grid = hr.GRIDS["41x23"]
    body = m.array("geom_bodyid")
    r0, g0 = hscan(e, "scanner", grid)
    seen = [int(g) for g in np.unique(g0[0]) if g >= 0 and body[g] > 0]
    g = max(seen, key=lambda k: int((g0[0] == k).sum())); bd = int(body[g])
    e.set_slot_active(bd, 0, env0=2, n=1)
    r1, g1 = hscan(e, "scanner", grid)
    assert not (g1[2] == g).any() and (g1[0] == g).any()
    for env in (0, 1, 3):
        assert np.array_equal(r1[env], r0[env]) and np.array_equal(g1[env], g0[env])
    check("inactive slot", r1[2], g1[2], device_scene(e, m, 2, visible=body != bd), sensor_rays(e, m, 0, 2, grid, "yaw"))
    e.set_slot_active(bd, 1, env0=2, n=1)
    r2, g2 = e.height_scan("scanner", **hr.kwargs(grid))
    assert np.array_equal(r2, r0) and np.array_equal(g2, g0)
    e.close()


# ------------------------------------------------------------------ 9. points
@pytest.mark.parametrize("align", hr.ALIGNS)
def test_points(prim, align):
    m, e, scene = prim
    grid = (41, 23, (0.17, 0.2), (0.3, -0.1), 0.5)      # (wider than the floor: some rays miss)
    r, g = e.height_scan("scanner", **hr.kwargs(grid), align=align, n=2)
    r3, g3, pts = e.height_scan("scanner", **hr.kwargs(grid), align=align, n=2, points=True)
    assert pts.dtype == np.float32 and pts.shape == r.shape + (3,)
    assert np.array_equal(bits(r3), bits(r)) and np.array_equal(g3, g), "range and geom id are the same bits with and without the points pointer"
    ref = hr.points64(grid, r3, g3)
    miss = g3 < 0
    assert miss.any() and (~miss).any()
    assert (pts[miss][:, 2] == np.float32(grid[4])).all(), "a miss is the ray's start point"
    err = np.abs(pts.astype(float) - ref).max(axis=-1) / np.maximum(1.0, np.abs(r3.astype(float)))
    print(f"points {align}: max scaled error {err.max():.3e}")
    assert err.max() <= TOL


# ------------------------------------------------------------------ 10. against mjh_ray fed the same rays
@pytest.mark.parametrize("align", hr.ALIGNS)
def test_against_the_ray_route(rig, align):
    m, e, bd = rig
    r, g = e.height_scan("head", **hr.kwargs(RIG_GRID), align=align, bodyexclude=bd)
    rays = [sensor_rays(e, m, 1, env, RIG_GRID, align) for env in range(NENV)]
    dist, gid = e.ray(np.array([p for p, _ in rays]), np.array([v for _, v in rays]), bodyexclude=bd)      # per_env rays, world frame
    body = m.array("geom_bodyid")
    same = 0
    for env in range(NENV):
        rob = rm.robust(rays[env], device_scene(e, m, env, visible=body != bd))
        r0, g0 = r[env].ravel(), g[env].ravel()
        assert (g0[rob] == gid[env][rob]).all()
        err = np.abs(r0.astype(float) - dist[env]) / np.maximum(1.0, np.abs(dist[env]))
        assert err[rob].max() <= TOL
        same += int((r0 == dist[env].astype(np.float32)).sum())
        print(f"ray route {align} env {env}: robust share {rob.mean():.4f}, max scaled difference {err[rob].max():.3e}")
    print(f"ray route {align}: {same} of {r.size} ranges bitwise equal")


# ------------------------------------------------------------------ 11. the device form
def test_device_form_same_bits(rig):
    import torch
    m, e, bd = rig
    grid = hr.GRIDS["9x70"]
    width, height = grid[:2]
    env0, n = 1, 3
    kw = dict(hr.kwargs(grid), align="base", env0=env0, n=n, bodyexclude=bd)
    r, g, pts = e.height_scan("head", points=True, **kw)
    dev = torch.device("cuda:0")
    tr = torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev); tg = torch.full((n, height, width), 7, dtype=torch.int32, device=dev)
    tp = torch.full((n, height, width, 3), 7.0, dtype=torch.float32, device=dev); t2 = torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    e.height_scan_device(tr.data_ptr(), tg.data_ptr(), tp.data_ptr(), "head", **kw)
    e.height_scan_device(t2.data_ptr(), None, None, 1, **kw)
    e.synchronize()
    assert np.array_equal(bits(tr.cpu().numpy()), bits(r)) and np.array_equal(tg.cpu().numpy(), g) and np.array_equal(bits(tp.cpu().numpy()), bits(pts))
    assert np.array_equal(bits(t2.cpu().numpy()), bits(r)), "without the geom-id and point images the range bits are the same"
    only_r = np.full((n, height, width), 7.0, dtype=np.float32)
    o = e._heightscan_options(1, width, height, grid[2], grid[3], grid[4], "base", dict(bodyexclude=bd))
    assert e.lib.mjh_heightscan(e.h, env0, n, C.byref(o), C.c_void_p(only_r.ctypes.data), None, None) == 0
    assert np.array_equal(bits(only_r), bits(r))


# ------------------------------------------------------------------ 12. nothing of the state is written
def test_no_side_effects(lib):
    m = prim_model(lib, gravity=(0, 0, -9.81), rig=True)
    a, b = ms.Engine(m, NENV), ms.Engine(m, NENV)
    a.step(150); b.step(150)      # (the free bodies have begun to land on the floor)
    before = _snapshot(a)
    bd = m.name2id(0, "rig")
    a.height_scan("head", **hr.kwargs(hr.GRIDS["9x70"])); a.height_scan("head", **hr.kwargs(hr.GRIDS["41x23"]), align="base", env0=1, n=2, cull=0, points=True, bodyexclude=bd, exclude_tree=1)
    for x, y in zip(before, _snapshot(a)):
        assert np.array_equal(x, y)
    a.step(3); b.step(3)
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "a step after a scan equals a step without one"
    # ... and between the halves of a split step, as mjh_ray
    a.step1(); r, g = a.height_scan("head", **hr.kwargs(hr.GRIDS["9x70"])); a.step2()
    b.step1(); b.get_geom_state(0, NENV); b.step2()
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "the call sequence rules are those of mjh_get_geom_state"
    assert (g >= 0).any()
    a.close(); b.close()


# ------------------------------------------------------------------ 13. errors
def test_errors_launch_nothing(prim, lib):
    m, e, scene = prim
    width, height = 9, 3
    kw = dict(width=width, height=height, spacing=(0.2, 0.3), offset=(0.1, 0.0), above=0.5)
    good_r, good_g, good_p = e.height_scan("scanner", points=True, **kw)
    rng_ = np.full((NENV, height, width), 7.0, dtype=np.float32); gid = np.full((NENV, height, width), 7, dtype=np.int32)
    pts = np.full((NENV, height, width, 3), 7.0, dtype=np.float32)

    def call(eng=e, env0=0, n=NENV, null=False, spacing=(0.2, 0.3), offset=(0.1, 0.0), **opt):
        o = capi.HeightScanOptions(); lib.mjh_heightscan_default_options(C.byref(o))
        o.site, o.width, o.height, o.above = 0, width, height, 0.5
        o.spacing[0], o.spacing[1] = spacing; o.offset[0], o.offset[1] = offset
        for k, v in opt.items():
            setattr(o, k, v)
        return lib.mjh_heightscan(eng.h, env0, n, C.byref(o), None if null else C.c_void_p(rng_.ctypes.data), C.c_void_p(gid.ctypes.data), C.c_void_p(pts.ctypes.data))

    def ok():
        assert (rng_ == 7.0).all() and (gid == 7).all() and (pts == 7.0).all(), "nothing was launched: the outputs are untouched"
        assert call() == 0
        assert np.array_equal(rng_, good_r) and np.array_equal(gid, good_g) and np.array_equal(pts, good_p)
        rng_[:] = 7.0; gid[:] = 7; pts[:] = 7.0

    for bad in (dict(site=1), dict(site=-2), dict(bodyexclude=m.nbody), dict(bodyexclude=-2), dict(exclude_tree=1), dict(align=3), dict(align=-1),
                dict(width=0), dict(height=0), dict(width=-3), dict(width=1 << 16, height=1 << 15),
                dict(spacing=(0.0, 0.3)), dict(spacing=(0.2, -1.0)), dict(spacing=(np.nan, 0.3)), dict(spacing=(0.2, np.inf)),
                dict(offset=(np.nan, 0.0)), dict(offset=(0.0, np.inf)), dict(offset=(1e39, 0.0)), dict(above=np.nan), dict(above=-np.inf),
                dict(spacing=(1e38, 0.3)), dict(env0=2, n=3), dict(env0=-1, n=2), dict(env0=NENV, n=1), dict(n=0), dict(null=True)):
        assert call(**bad) == MJH_ERR_ARG, bad
        assert lib.mjh_last_error()
        ok()
    assert lib.mjh_heightscan_device(e.h, 0, NENV, None, None, None, None) == MJH_ERR_ARG
    ok()
    with pytest.raises(MjhError):
        e.height_scan("scanner", 0, 8, 0.1)
    with pytest.raises(ValueError):
        e.height_scan("no such site", 8, 8, 0.1)
    with pytest.raises(ValueError):
        e.height_scan("scanner", 8, 8, 0.1, align="pitch")
    with pytest.raises(TypeError):
        e.height_scan("scanner", 8, 8, 0.1, per_env=1)
    ok()
