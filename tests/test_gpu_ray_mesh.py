"""Rays against mesh geoms on the device (mjh_ray / mjh_ray_device in mesh mode 1) against the fp64 reference of ray_mesh_ref.py:
scipy's hull of the model's kept vertices, intersected triangle by triangle, merged with ray_ref.cast for every other geom type.

As in test_gpu_ray.py the reference is fed the device's own geom poses (mjh_get_geom_state), so only the ray arithmetic is under test, and
the tolerance is that file's: on robust rays (same geom, distance within 1e-3 under 1e-4 shifts of the origin) the geom ids are equal and
|dist - ref| <= 5e-5 max(1, dist) — scene coordinates of at most 5 m give an fp32 ulp near 5e-7, robustness bounds the conditioning at
10, ten times that is the tolerance; a hull plane rounded to float32 moves by 6e-8 of the mesh's size, far inside it.  The share of
non-robust rays stays within 10 % (checked beforehand on the CPU with the oracle's poses of the same states: 0 .. 3 %).

Measured on an MI355X: every case within 3.5e-7 scaled on its robust rays, non-robust shares 0 .. 3.1 %."""
import numpy as np
import pytest

import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr
from mujoco_sim_amd.engine import MjhError

pytestmark = pytest.mark.gpu

TOL = 5e-5


def _check(name, dist, gid, scene, rays, cutoff=0.0):
    """dist / gid of ONE env against the reference on the robust rays; returns the largest scaled error"""
    ref_d, ref_g = rm.cast(rays[0], rays[1], scene, cutoff=cutoff)
    rob = rm.robust(rays, scene)
    share = 1.0 - rob.mean()
    hit = rob & (ref_g >= 0)
    err = np.abs(dist - ref_d) / np.maximum(1.0, np.abs(ref_d))
    worst = float(err[hit].max()) if hit.any() else 0.0
    print(f"{name}: {len(rob)} rays, non-robust share {share:.3f}, hits {int(hit.sum())}, max scaled error {worst:.3e}")
    assert share <= 0.10, name
    assert (gid[rob] == ref_g[rob]).all(), name
    miss = rob & (ref_g < 0)
    assert (dist[miss] == -1.0).all() and (gid[miss] == -1).all(), name
    assert worst <= TOL, name
    return worst


def _device_scene(e, m, env, tris, visible=None):
    gp, gm = e.get_geom_state(env, 1)
    sc = rr.scene_from_device(gp[0], gm[0], m.array("geom_size"), m.array("geom_type"), visible)
    return rm.attach_meshes(sc, m, tris)


def _tris(m):
    return [rm.hull_triangles(v) for v in rm.model_mesh_verts(m)]


# ------------------------------------------------------------------ 4. the box-mesh model of the mode-0 skip test
def test_box_mesh_model_mode_switch(lib):
    m = rr.mesh_model(lib)
    assert m.ray_skipped_geoms() == 2, "the mode-0 count keeps its meaning"
    e = ms.Engine(m, 4)
    assert e.ray_mesh_mode == 0
    types = m.array("geom_type")
    gp, _ = e.get_geom_state(0, 1)
    mesh = np.nonzero(types == rr.MESH)[0]
    ball = int(np.nonzero(types == rr.SPHERE)[0][0])
    # the three rays of test_gpu_ray.py::test_mesh_geoms_are_skipped, then one from the first mesh's centre
    P = np.array([gp[0, mesh[0]] + [0, 0, 1.0], gp[0, mesh[1]] + [0, 0, 1.0], gp[0, mesh[0]] + [-1.0, 0, 0], gp[0, mesh[0]]])
    V = np.array([[0, 0, -1.0], [0, 0, -1.0], [1.0, 0, 0], [0, 0, -1.0]])
    d0, g0 = e.ray(P, V)
    assert list(g0[0, :3]) == [ball, 0, -1]
    e.ray_mesh_mode = 1
    assert e.ray_mesh_mode == 1
    d1, g1 = e.ray(P, V)
    scene = _device_scene(e, m, 0, _tris(m))
    _check("box mesh model", d1[0], g1[0], scene, (P, V))
    # the mesh body stands unrotated at z = 1.0 and the box is 0.2 x 0.15 x 0.1 (half extents): from 1.0 above its centre straight down
    # the top face is 1.0 - 0.1 away, from the centre the far (bottom) face 0.1, and from 1.0 beside it along x the near side face 1.0 - 0.2
    assert list(g1[0]) == [mesh[0], mesh[1], mesh[0], mesh[0]]
    assert d1[0, 0] == pytest.approx(0.9, abs=1e-5) and d1[0, 1] == pytest.approx(0.9, abs=1e-5)
    assert d1[0, 2] == pytest.approx(0.8, abs=1e-5) and d1[0, 3] == pytest.approx(0.1, abs=1e-5)
    for env in range(1, 4):
        assert np.array_equal(d1[env], d1[0]) and np.array_equal(g1[env], g1[0])
    with pytest.raises(MjhError):
        e.ray_mesh_mode = 2
    assert lib.mjh_ray_set_mesh_mode(e.h, -1) == -1 and e.ray_mesh_mode == 1, "a bad mode changes nothing"
    e.ray_mesh_mode = 0
    d2, g2 = e.ray(P, V)
    assert np.array_equal(d2.view(np.uint64), d0.view(np.uint64)) and np.array_equal(g2, g0), "mode 0 again: bitwise the skip test's results"
    assert not np.isin(g2, mesh).any()
    e.close()


# ------------------------------------------------------------------ 5. meshes and primitives, a pose per env
@pytest.fixture(scope="module")
def mixed(lib):
    m, bodies, site = rm.mixed_model(lib)
    e = ms.Engine(m, 4)
    e.ray_mesh_mode = 1
    q = rm.mixed_qpos(m, 4)
    e.set_state(qpos=q, qvel=np.zeros((4, m.nv)))
    tris = _tris(m)
    scenes = [_device_scene(e, m, i, tris) for i in range(4)]
    rays = rm.make_rays(21, scenes[0], 130, rm.MIXED_ORIGIN_LO, rm.MIXED_ORIGIN_HI)
    yield dict(m=m, e=e, bodies=bodies, site=site, scenes=scenes, rays=rays, tris=tris)
    e.close()


@pytest.mark.parametrize("nray", [1, 63, 65, 130])
def test_mixed_scene_shared_rays(mixed, nray):
    e, scenes = mixed["e"], mixed["scenes"]
    rays = (mixed["rays"][0][:nray], mixed["rays"][1][:nray])
    dist, gid = e.ray(*rays)
    assert dist.shape == (4, nray)
    for env in range(4):
        _check(f"mixed nray {nray} env {env}", dist[env], gid[env], scenes[env], rays)
    if nray == 130:
        types = scenes[0]["type"]
        for env in range(4):
            assert {int(types[g]) for g in gid[env] if g >= 0} >= {rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.ELLIPSOID, rr.CYLINDER, rr.BOX, rr.MESH}
        assert not np.array_equal(dist[0], dist[1]), "a pose per env: the scans differ"
        hit_meshes = {int(g) for g in gid.ravel() if g >= 0 and types[g] == rr.MESH}
        assert len(hit_meshes) == 4, "all three mesh assets (and the static geom) are hit"


def test_mixed_scene_per_env_rays(mixed):
    """a ray set per env, each aimed at that env's own poses: a wrong env index (rays or poses) shows"""
    e, scenes = mixed["e"], mixed["scenes"]
    sets = [rm.make_rays(31 + i, scenes[i], 65, rm.MIXED_ORIGIN_LO, rm.MIXED_ORIGIN_HI) for i in range(4)]
    P = np.stack([s[0] for s in sets]); V = np.stack([s[1] for s in sets])
    dist, gid = e.ray(P, V)
    for env in range(4):
        _check(f"mixed per-env rays env {env}", dist[env], gid[env], scenes[env], sets[env])
    d13, g13 = e.ray(P[1:3], V[1:3], env0=1, n=2)
    assert np.array_equal(d13, dist[1:3]) and np.array_equal(g13, gid[1:3])


def test_mixed_scene_site_frame_on_a_mesh_body(mixed):
    m, e, scenes = mixed["m"], mixed["e"], mixed["scenes"]
    bd, site = mixed["bodies"][0], mixed["site"]
    rng = np.random.default_rng(5)
    nray = 65
    V = rng.normal(size=(nray, 3)); V /= np.linalg.norm(V, axis=1, keepdims=True)
    P, V = rr.f32(rng.uniform(-0.02, 0.02, size=(nray, 3)), V * rng.uniform(0.5, 2.0, size=(nray, 1)))
    dist, gid = e.ray(P, V, site=site)
    xp, xq = e.get_body_state()
    Rs = rr.quat2mat(rm.MIXED_SITE_QUAT).reshape(3, 3)
    types = scenes[0]["type"]
    seen = set()
    for i in range(4):
        Rb = rr.quat2mat(xq[i, bd]).reshape(3, 3)
        Pw = xp[i, bd] + Rb @ np.asarray(rm.MIXED_SITE_POS) + P @ (Rb @ Rs).T
        Vw = V @ (Rb @ Rs).T
        _check(f"mixed site frame env {i}", dist[i], gid[i], scenes[i], (Pw, Vw))
        seen |= {int(types[g]) for g in gid[i] if g >= 0}
    assert rr.MESH in seen and len(seen) >= 3
    assert not np.array_equal(gid[0], gid[1]), "the site follows each env's own body"


# ------------------------------------------------------------------ 6. more geoms than one staging pass, one asset shared by 70 geoms
def test_mesh_geoms_beyond_one_staging_pass(lib):
    m, spec = rm.tetra_field_model(lib)
    types = m.array("geom_type")
    assert m.ngeom > 64 and (types == rr.MESH).sum() == 70 and m.c.nmesh == 1 and m.c.nmeshplane == 4
    e = ms.Engine(m, 2)
    e.ray_mesh_mode = 1
    scene = _device_scene(e, m, 0, _tris(m))
    rays = rm.make_rays(43, scene, 96, (-3.0, -3.0, 0.05), (3.0, 3.0, 3.0))
    dist, gid = e.ray(*rays)
    assert np.array_equal(dist[1], dist[0]) and np.array_equal(gid[1], gid[0])
    _check("tetrahedron field", dist[0], gid[0], scene, rays)
    g = gid[0]
    second = (g >= 64) & (types[np.maximum(g, 0)] == rr.MESH)
    first = (g >= 0) & (g < 64) & (types[np.maximum(g, 0)] == rr.MESH)
    assert second.sum() >= 5 and first.sum() >= 5, "mesh geoms of both staging passes are hit"
    assert (types[g[g >= 0]] == rr.SPHERE).any()
    e.close()


# ------------------------------------------------------------------ 7. options and slots apply to mesh geoms
def test_options_on_meshes(mixed):
    m, e, scenes, rays = mixed["m"], mixed["e"], mixed["scenes"], mixed["rays"]
    body, types = m.array("geom_bodyid"), m.array("geom_type")
    scene = scenes[0]
    d0, g0 = e.ray(*rays, n=1)
    # bodyexclude of a mesh body some ray hits
    hit_mesh = [int(g) for g in g0[0] if g >= 0 and types[g] == rr.MESH and body[g] > 0]
    assert hit_mesh
    bx = int(body[hit_mesh[0]])
    d1, g1 = e.ray(*rays, n=1, bodyexclude=bx)
    _check("bodyexclude mesh body", d1[0], g1[0], dict(scene, visible=body != bx), rays)
    was = (g0[0] >= 0) & (body[np.maximum(g0[0], 0)] == bx)
    assert was.any() and not (body[g1[0][g1[0] >= 0]] == bx).any()
    assert np.array_equal(d1[0][~was], d0[0][~was]) and np.array_equal(g1[0][~was], g0[0][~was]), "exactly that body's geoms are hidden"
    # flg_static = 0 hides the static mesh geom: a ray straight down onto it
    gs = int(np.nonzero((types == rr.MESH) & (body == 0))[0][0])
    P = np.array([scene["pos"][gs] + [0.01, 0.02, 1.0]]); V = np.array([[0, 0, -1.0]])
    da, ga = e.ray(P, V, n=1)
    db, gb = e.ray(P, V, n=1, flg_static=0)
    assert ga[0, 0] == gs and gb[0, 0] == -1 and db[0, 0] == -1.0, "through the static mesh and the (static) floor"
    d2, g2 = e.ray(*rays, n=1, flg_static=0)
    _check("flg_static 0", d2[0], g2[0], dict(scene, visible=body != 0), rays)
    assert (body[g2[0][g2[0] >= 0]] != 0).all()
    # cutoff: the hit on the static mesh lies between 0.5 and 1.0 away
    assert 0.5 < da[0, 0] < 1.0
    for cut, want in ((0.0, gs), (0.5, -1), (1.0, gs)):
        d, g = e.ray(P, V, n=1, cutoff=cut)
        assert g[0, 0] == want and (d[0, 0] == da[0, 0] if want >= 0 else d[0, 0] == -1.0), cut


def test_inactive_slot_hides_a_mesh_body_in_that_env_only(mixed):
    m, e, scenes = mixed["m"], mixed["e"], mixed["scenes"]
    body = m.array("geom_bodyid")
    bd = mixed["bodies"][2]
    g = int(np.nonzero(body == bd)[0][0])
    # per-env rays: straight down onto each env's own copy of the mesh geom
    P = np.stack([[scenes[i]["pos"][g] + [0, 0, 1.0]] for i in range(4)]); V = np.tile([[[0, 0, -1.0]]], (4, 1, 1))
    d0, g0 = e.ray(P, V)
    assert (g0[:, 0] == g).all()
    e.set_slot_active(bd, 0, env0=1, n=1)
    try:
        d1, g1 = e.ray(P, V)
        assert g1[1, 0] != g and d1[1, 0] != d0[1, 0], "env 1's ray passes through"
        keep = [0, 2, 3]
        assert np.array_equal(g1[keep], g0[keep]) and np.array_equal(d1[keep], d0[keep]), "env 0's (and 2's, 3's) does not"
        rd, rg = rm.cast(P[1], V[1], dict(scenes[1], visible=body != bd))
        assert g1[1, 0] == rg[0] and d1[1, 0] == pytest.approx(rd[0], abs=TOL * max(1.0, abs(rd[0])))
    finally:
        e.set_slot_active(bd, 1, env0=1, n=1)
    d2, g2 = e.ray(P, V)
    assert np.array_equal(g2, g0) and np.array_equal(d2, d0)


# ------------------------------------------------------------------ 8. bitwise: mesh-free models, the device entry point
def test_mode_1_on_a_mesh_free_model_is_bitwise_mode_0(lib):
    m = rm.primitives_model(lib)
    assert m.c.nmesh == 0 and m.c.nmeshplane == 0
    e = ms.Engine(m, 4)
    gp, gm = e.get_geom_state(0, 1)
    scene = rr.scene_from_device(gp[0], gm[0], m.array("geom_size"), m.array("geom_type"))
    rays = rr.primitive_rays(scene, 130)
    d0, g0 = e.ray(*rays)
    e.ray_mesh_mode = 1
    d1, g1 = e.ray(*rays)
    assert np.array_equal(d1.view(np.uint64), d0.view(np.uint64)) and np.array_equal(g1, g0)
    assert (g0 >= 0).sum() > 200
    e.close()


def test_ray_device_in_mode_1_same_bits(mixed):
    import torch
    e, rays = mixed["e"], mixed["rays"]
    assert e.ray_mesh_mode == 1
    P, V = rays
    n, nray = 3, len(P)
    dist, gid = e.ray(P, V, env0=1, n=n)
    dev = torch.device("cuda:0")
    tp = torch.tensor(P, dtype=torch.float32, device=dev).contiguous(); tv = torch.tensor(V, dtype=torch.float32, device=dev).contiguous()
    td = torch.full((n, nray), 7.0, dtype=torch.float32, device=dev); tg = torch.full((n, nray), 7, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    e.ray_device(tp.data_ptr(), tv.data_ptr(), td.data_ptr(), tg.data_ptr(), nray, env0=1, n=n)
    e.synchronize()
    assert np.array_equal(td.cpu().numpy().view(np.uint32), dist.astype(np.float32).view(np.uint32))
    assert np.array_equal(tg.cpu().numpy(), gid)
    assert np.array_equal(dist.astype(np.float32).astype(np.float64), dist), "mjh_ray returns the device's fp32 results"
    types = mixed["scenes"][0]["type"]
    assert (types[gid[gid >= 0]] == rr.MESH).any()


# ------------------------------------------------------------------ 9. PR2 with its meshes
def test_pr2_fan(lib):
    m = rm.load_robot(lib, "pr2")
    types = m.array("geom_type")
    assert (types == rr.MESH).sum() == 37 and m.ngeom == 55 and m.c.nmeshplane > 1000
    e = ms.Engine(m, 2)
    e.ray_mesh_mode = 1
    tris = _tris(m)
    rays = rm.pr2_fan()
    assert len(rays[0]) == 128
    dist, gid = e.ray(*rays)
    for env in range(2):
        _check(f"pr2 fan env {env}", dist[env], gid[env], _device_scene(e, m, env, tris), rays)
    hits = gid[0][gid[0] >= 0]
    assert len(hits) >= 60 and (types[hits] == rr.MESH).sum() > len(hits) / 2, "more than half of the hits are mesh geoms"
    e.ray_mesh_mode = 0
    _, g0 = e.ray(*rays, n=1)
    assert not (types[g0[0][g0[0] >= 0]] == rr.MESH).any(), "mode 0 sees the primitives only"
    e.close()
