"""RGB-D images on the device (mjh_render / mjh_render_device, csrc/render.hip) against the fp64 reference tests/render_ref.py, by the
comparison of tests/render_check.py: on the pixels the reference finds robust and feature-robust (at most 2 % of an image are left
out, asserted) the geom ids agree, max_c |n - n_ref| <= TOL_N = 4 N_HOST = 2.6e-5 (N_HOST: the host build of the same code against
the same reference, tests/test_render_host.py) and every colour channel is within 1 + ceil(255 diffuse sqrt(3) TOL_N) = 2 levels; a
miss is normal (0, 0, 0) and the background colour exactly; with ambient = 1, diffuse = 0 every hit is the level of its geom's colour
bit for bit.  The reference works from the device's own poses (mjh_get_body_state, mjh_get_geom_state): only the image arithmetic is
under test.  4 envs, images of at most 30 x 20 pixels.

Measured on one MI355X (`pytest tests/test_gpu_render.py -m gpu -s` prints every case): worst max_c |n - n_ref| 1.25e-5 (the camera
on a free body, own body hidden, env 3), primitives 4.6e-6 .. 9.1e-6, many spheres 9.1e-6, height field 1.2e-7 (from above; from below, base and walls), hulls 1.5e-7, triangles
9.6e-8; colour difference 0 levels in every compared pixel; largest excluded share 1.56 % (side view 8 x 8: one pixel of 64)."""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
import ray_ref as rr
import render_check as rc
import render_ref as rf
from mujoco_sim_amd import capi
from mujoco_sim_amd.engine import MjhError
from render_check import NENV, check_render

pytestmark = pytest.mark.gpu

MJH_ERR_ARG = -1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.ascontiguousarray(a)


def same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def prim(lib):
    m = rc.prim_model(lib)
    e = ms.Engine(m, NENV)
    yield m, e, rc.device_scene(e, m, 0)
    e.close()


# ------------------------------------------------------------------ 1. every primitive type, both views, tile edges
@pytest.mark.parametrize("cam", ["front", "side"])
@pytest.mark.parametrize("width,height", [(30, 20), (8, 8), (9, 8), (1, 1)])
def test_primitives(prim, cam, width, height):
    m, e, scene = prim
    depth, gid, nrm, col = e.render(cam, width, height)
    assert depth.shape == gid.shape == (NENV, height, width) and nrm.shape == (NENV, height, width, 3) and col.shape == (NENV, height, width, 4)
    assert nrm.dtype == np.float32 and col.dtype == np.uint8
    rays = rc.camera_rays(e, m, m.name2id(5, cam), 0, width, height)
    check_render(f"primitives {cam} {width}x{height}", depth[0], gid[0], nrm[0], col[0], scene, rays, rc.model_colours(m))
    for env in range(1, NENV):      # no per-env data: every env sees the same scene
        assert same((depth[env], gid[env], nrm[env], col[env]), (depth[0], gid[0], nrm[0], col[0]))
    if (width, height) == (30, 20):
        assert {int(scene["type"][g]) for g in gid[0].ravel() if g >= 0} >= {rr.PLANE, rr.SPHERE, rr.CAPSULE, rr.ELLIPSOID, rr.CYLINDER, rr.BOX}
        assert (gid[0] < 0).any(), "the view has misses too"


# ------------------------------------------------------------------ 2. depth and geom id are mjh_depth's bits; range, cutoff
def test_depth_and_geomid_are_mjh_depth_bits(prim):
    m, e, scene = prim
    width, height = 30, 20
    rays = rc.camera_rays(e, m, 0, 0, width, height)
    norm = np.linalg.norm(rays[1], axis=1)
    ref_d = rf.cast(rays[0], rays[1], scene)[0]
    cut = 0.5 * (ref_d[ref_d >= 0].min() + ref_d[ref_d >= 0].max())
    bg = (0.1, 0.2, 0.3, 0.4)
    for kw in (dict(), dict(range=1), dict(cutoff=cut), dict(range=1, cutoff=float((ref_d * norm)[ref_d >= 0].mean())), dict(cull=0), dict(flg_static=0)):
        d, g = e.depth("front", width, height, **kw)
        depth, gid, nrm, col = e.render("front", width, height, background=bg, **kw)
        assert same((depth, gid), (d, g)), kw
        miss = gid < 0
        assert miss.any() and (nrm[miss] == 0.0).all() and (col[miss] == rf.level(np.asarray(bg, np.float32))).all(), kw
    depth, gid, nrm, col = e.render("front", width, height, n=1, cutoff=cut, background=bg)
    d0, g0, n0, c0 = e.render("front", width, height, n=1, background=bg)
    far = d0[0] > np.float32(cut)
    assert far.any() and (g0[0][far] >= 0).any() and (gid[0][far] == -1).all(), "a pixel beyond the cutoff is a miss"
    assert (nrm[0][far] == 0.0).all() and (col[0][far] == rf.level(np.asarray(bg, np.float32))).all(), "... with the zero normal and the background colour"
    assert same((nrm[0][~far], col[0][~far]), (n0[0][~far], c0[0][~far])), "the rest is unchanged"
    check_render("primitives front, cutoff", depth[0], gid[0], nrm[0], col[0], scene, rays, rc.model_colours(m), background=bg, cutoff=cut)
    dr, gr, nr, cr = e.render("front", width, height, n=1, range=1)
    check_render("primitives front, range 1", dr[0], gr[0], nr[0], cr[0], scene, rays, rc.model_colours(m), scale=norm)


# ------------------------------------------------------------------ 3. a camera on a free body, inside its own sphere, a pose per env
def test_camera_inside_its_own_sphere_and_per_env_poses(lib):
    m = rc.prim_model(lib, gravity=(0, 0, -9.81), rig=True)
    e = ms.Engine(m, NENV)
    rng = np.random.default_rng(23)
    bd = m.name2id(0, "rig")
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[bd]])
    q = np.tile(m.array("qpos0"), (NENV, 1))
    Rc = rr.quat2mat(rc.RIG_CAM_QUAT).reshape(3, 3)
    for i in range(NENV):
        eye = np.array([rng.uniform(-1.5, 1.5), rng.uniform(-4.2, -3.2), rng.uniform(2.0, 3.2)])
        Rw = rc.look_at(eye, np.array([0.0, 0.0, 0.8]) + rng.uniform(-0.4, 0.4, size=3))
        Rb = Rw @ Rc.T
        q[i, adr:adr + 3] = eye - Rb @ np.array(rc.RIG_CAM_POS)
        q[i, adr + 3:adr + 7] = rc.mat2quat(Rb)
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv)))
    e.step(5)      # a few steps under gravity: every body has moved, each env from its own pose
    width, height = 30, 20
    body = m.array("geom_bodyid")
    rigg = m.name2id(2, "rigg")
    inside = e.render("eye", width, height)
    outside = e.render("eye", width, height, bodyexclude=bd)
    for env in range(NENV):
        rays = rc.camera_rays(e, m, 2, env, width, height)
        scene = rc.device_scene(e, m, env)
        check_render(f"rig env {env} (from inside)", *(x[env] for x in inside), scene, rays, rc.model_colours(m))
        assert (inside[1][env] == rigg).all()
        hit = rays[0] + inside[0][env].reshape(-1, 1).astype(float) * rays[1]
        inward = (scene["pos"][rigg] - hit) / rc.RIG_RADIUS
        assert np.abs(inside[2][env].reshape(-1, 3) - inward).max() < 1e-4, "a camera inside a sphere gets the inward normal of the far surface"
        check_render(f"rig env {env} (own body hidden)", *(x[env] for x in outside), rc.device_scene(e, m, env, visible=body != bd), rays, rc.model_colours(m))
        assert (outside[1][env] >= 0).mean() > 0.3
    assert not np.array_equal(outside[3][0], outside[3][1]) and not np.array_equal(outside[2][0], outside[2][1]), "every env has its own image"
    e.close()


# ------------------------------------------------------------------ 4. many distinct winners per tile, misses, geoms of both staging passes
def test_many_spheres_from_above(lib):
    m = rc.spheres_model(lib)
    e = ms.Engine(m, NENV)
    scene = rc.device_scene(e, m, 0)
    width, height = 16, 16
    rays = rc.camera_rays(e, m, 0, 0, width, height)
    cut = 4.9      # most spheres lie within it, the floor (from 5.0 on) beyond: a miss
    out = e.render("above", width, height, cutoff=cut, background=(1.0, 1.0, 1.0, 1.0))
    check_render("many spheres 16x16, cutoff", *(x[0] for x in out), scene, rays, rc.model_colours(m), background=(1.0, 1.0, 1.0, 1.0), cutoff=cut)
    assert (out[1][0] < 0).any() and (out[1][0] > 0).any(), "spheres and misses"
    full = e.render("above", width, height, n=1)
    check_render("many spheres 16x16", *(x[0] for x in full), scene, rays, rc.model_colours(m))
    gid = full[1][0]
    assert (gid >= 64).any() and ((gid >= 0) & (gid < 64)).any(), "geoms of both staging passes of the depth launch are seen"
    tiles = [len(set(gid[i:i + 8, j:j + 8].ravel().tolist())) for i in (0, 8) for j in (0, 8)]
    print(f"distinct winning geoms per tile: {tiles}")
    assert min(tiles) >= 5, "every tile holds many distinct winners"
    for env in range(1, NENV):
        assert same(tuple(x[env] for x in out), tuple(x[0] for x in out))
    e.close()


# ------------------------------------------------------------------ 5. height field: top, wall, base
def test_hfield(lib):
    m = rc.hfield_model(lib)
    e = ms.Engine(m, NENV)
    scene = rc.device_scene(e, m, 0)
    rays = rc.camera_rays(e, m, 0, 0, 30, 20)
    out = e.render("cam", 30, 20)
    check_render("hfield 30x20", *(x[0] for x in out), scene, rays, rc.model_colours(m))
    _, ref_g, _, feat = rf.cast(rays[0], rays[1], scene)
    f = feat[ref_g == 0]
    print(f"hfield: top-triangle pixels {int((f >= 0).sum())} on {len(set(f[f >= 0].tolist()))} triangles, wall pixels {int((f <= -2).sum())}, base pixels {int((f == -1).sum())}")
    assert (f >= 0).sum() > 50 and len(set(f[f >= 0].tolist())) >= 6 and (f <= -2).any(), "top triangles and a wall are in view"
    for env in range(1, NENV):
        assert same(tuple(x[env] for x in out), tuple(x[0] for x in out))
    # the base, and the walls from outside: the camera under the field
    rays = rc.camera_rays(e, m, 1, 0, 30, 20)
    under = e.render("under", 30, 20)
    check_render("hfield from below 30x20", *(x[0] for x in under), scene, rays, rc.model_colours(m))
    _, ref_g, _, feat = rf.cast(rays[0], rays[1], scene)
    f = feat[ref_g == 0]
    print(f"hfield from below: base pixels {int((f == -1).sum())}, wall pixels {int((f <= -2).sum())}, top-triangle pixels {int((f >= 0).sum())}")
    assert (f == -1).sum() > 50 and (f <= -2).sum() > 20, "the base and a wall are in view"
    got = under[1][0].ravel() == 0
    base = got & (ref_g == 0) & (feat == -1)
    down = scene["mat"][0].reshape(3, 3) @ np.array([0.0, 0.0, -1.0])
    assert base.sum() > 50 and np.abs(under[2][0].reshape(-1, 3)[base] - down).max() < 1e-6, "the base's normal is the field's -z, towards the camera below"
    for env in range(1, NENV):
        assert same(tuple(x[env] for x in under), tuple(x[0] for x in under))
    e.close()


# ------------------------------------------------------------------ 6. mesh geoms: hulls and triangles
def test_mesh_hulls_and_triangles(lib):
    m, (g_torus, g_jaw, g_quad) = rc.meshes_model(lib)
    e = ms.Engine(m, NENV)
    width, height = 24, 16
    rays = rc.camera_rays(e, m, 0, 0, width, height)
    d0, g0, n0, c0 = e.render("cam", width, height)
    assert not np.isin(g0, [g_torus, g_jaw, g_quad]).any(), "mesh mode 0: no ray sees a mesh geom"
    check_render("meshes, mode 0", d0[0], g0[0], n0[0], c0[0], rc.device_scene(e, m, 0), rays, rc.model_colours(m))
    e.ray_mesh_mode = 1
    hull = e.render("cam", width, height)
    check_render("meshes, hulls", *(x[0] for x in hull), rc.device_scene(e, m, 0, surface=0), rays, rc.model_colours(m))
    e.ray_mesh_surface = 1
    tri = e.render("cam", width, height)
    check_render("meshes, triangles", *(x[0] for x in tri), rc.device_scene(e, m, 0, surface=1), rays, rc.model_colours(m))
    through = (tri[1][0] == 0) & (hull[1][0] == g_torus)
    assert through.any(), "the triangles let the camera see the floor through the torus's hole, which the hull fills"
    assert np.abs(tri[2][0][through] - np.float32([0, 0, 1])).max() < 1e-6, "there the normal is the floor's"
    assert np.abs(hull[2][0][through] - tri[2][0][through]).max() > 0.1, "and the hull's (the tilted flat top) differs"
    assert (tri[1][0] == g_quad).any() and not (hull[1][0] == g_quad).any(), "a mesh without volume has no hull"
    assert (tri[1][0] == g_torus).any() and (tri[1][0] == g_jaw).any()
    for env in range(1, NENV):
        assert same(tuple(x[env] for x in tri), tuple(x[0] for x in tri))
    e.ray_mesh_surface = 0; e.ray_mesh_mode = 0
    assert same(e.render("cam", width, height), (d0, g0, n0, c0)), "switching back is bitwise"
    e.close()


# ------------------------------------------------------------------ 7. per-env geom sizes, an inactive slot
def test_per_env_sizes_and_an_inactive_slot(lib):
    m = rc.prim_model(lib)
    e = ms.Engine(m, NENV)
    size = m.array("geom_size")
    small = (0.8 * size).astype(np.float32).astype(float)
    e.set_env_param("geom_size", small[None, :], env0=1)
    body = m.array("geom_bodyid")
    bg = (0.0, 1.0, 0.0, 1.0)
    base = e.render("front", 30, 20, background=bg)
    seen = [int(g) for g in np.unique(base[1][0]) if g >= 0 and body[g] > 0]
    g = max(seen, key=lambda k: int((base[1][0] == k).sum())); bd = int(body[g])
    e.set_slot_active(bd, 0, env0=2, n=1)
    out = e.render("front", 30, 20, background=bg)
    for env in range(NENV):
        scene = rc.device_scene(e, m, env, size=small if env == 1 else size, visible=(body != bd) if env == 2 else None)
        check_render(f"per-env sizes / slot, env {env}", *(x[env] for x in out), scene, rc.camera_rays(e, m, 0, env, 30, 20), rc.model_colours(m), background=bg)
    assert not np.array_equal(out[2][1], out[2][0]) and same(tuple(x[3] for x in out), tuple(x[0] for x in out))
    assert not (out[1][2] == g).any() and (out[1][0] == g).any()
    gone = (base[1][2] == g) & (out[1][2] < 0)
    print(f"inactive slot: geom {g} held {int((base[1][2] == g).sum())} pixels, {int(gone.sum())} of them now show the background")
    assert (out[3][2][gone] == rf.level(np.asarray(bg, np.float32))).all(), "where only the hidden body was, that env shows the background"
    assert same(tuple(x[0] for x in out), tuple(x[0] for x in base)) and same(tuple(x[1] for x in out), tuple(x[1] for x in base))
    e.close()


# ------------------------------------------------------------------ 8. flat colours are exact; builder and MJCF colours agree
MJCF_COLOURS = {"ball": (0.8, 0.2, 0.1, 1.0), "crate": (0.15, 0.55, 0.95, 0.3)}


def _colour_models(lib):
    from helpers import D, set_opt
    view = ((1.5, -2.0, 1.6), (0.0, 0.0, 0.3), 50.0)
    quat = rc.mat2quat(rc.look_at(view[0], view[1]))
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, -9.81])
    g = lib.mjh_builder_add_geom(b, b"floor", 0, rr.PLANE, D(1.0, 1.0, 0.05), None, None, None, -1, -1, -1, -1)
    assert lib.mjh_builder_set_geom_rgba(b, g, D(0.4, 0.4, 0.4, 1.0)) == 0
    g = lib.mjh_builder_add_geom(b, b"ball", 0, rr.SPHERE, D(0.25, 0, 0), D(0.3, 0.2, 0.25), None, None, -1, -1, -1, -1)
    assert lib.mjh_builder_set_geom_rgba(b, g, D(*MJCF_COLOURS["ball"])) == 0
    g = lib.mjh_builder_add_geom(b, b"crate", 0, rr.BOX, D(0.2, 0.15, 0.3), D(-0.4, -0.1, 0.3), None, None, -1, -1, -1, -1)
    assert lib.mjh_builder_set_geom_rgba(b, g, D(*MJCF_COLOURS["crate"])) == 0
    g = lib.mjh_builder_add_geom(b, b"plain", 0, rr.CAPSULE, D(0.08, 0.2, 0), D(0.7, 0.5, 0.3), None, None, -1, -1, -1, -1)
    bd = lib.mjh_builder_add_body(b, b"far", 0, D(0, 0, 50.0), None, 0.0)
    lib.mjh_builder_add_joint(b, b"farj", bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"fg", bd, rr.SPHERE, D(0.05, 0, 0), None, None, None, -1, -1, -1, -1)
    assert lib.mjh_builder_add_camera(b, b"cam", 0, D(*view[0]), D(*quat), view[2]) == 0
    built = rc.compile_model(lib, b)
    r = lambda xs: " ".join(repr(float(x)) for x in xs)
    xml = f"""<mujoco>
      <default>
        <default class="ball"><geom rgba="{r(MJCF_COLOURS['ball'])}"/></default>
        <default class="crate"><geom rgba="{r(MJCF_COLOURS['crate'])}"/></default>
      </default>
      <asset><material name="floor" rgba="0.4 0.4 0.4 1"/></asset>
      <worldbody>
        <geom name="floor" type="plane" size="1 1 0.05" material="floor"/>
        <geom name="ball" class="ball" type="sphere" size="0.25" pos="0.3 0.2 0.25"/>
        <geom name="crate" class="crate" type="box" size="0.2 0.15 0.3" pos="-0.4 -0.1 0.3"/>
        <geom name="plain" type="capsule" size="0.08 0.2" pos="0.7 0.5 0.3"/>
        <body name="far" pos="0 0 50"><freejoint name="farj"/><geom name="fg" type="sphere" size="0.05"/></body>
        <camera name="cam" pos="{r(view[0])}" quat="{r(quat)}" fovy="{view[2]}"/>
      </worldbody>
    </mujoco>"""
    loaded = ms.load_mjcf(xml)
    return built, loaded


def test_flat_colours_are_exact_and_builder_and_mjcf_agree(lib, prim):
    m, e, scene = prim
    bg = (0.25, 0.5, 0.75, 1.0)
    for cam, w, h in (("front", 30, 20), ("side", 9, 8)):
        depth, gid, nrm, col = e.render(cam, w, h, ambient=1.0, diffuse=0.0, background=bg)
        assert (gid >= 0).any() and (gid < 0).any()
        assert np.array_equal(col, rc.flat_colours(rc.model_colours(m), gid, bg)), "ambient 1, diffuse 0: every hit pixel is its geom's colour, bit for bit"
    built, loaded = _colour_models(lib)
    assert np.array_equal(built.array("geom_rgba"), loaded.array("geom_rgba")) and np.array_equal(built.array("geom_type"), loaded.array("geom_type"))
    assert built.array("geom_rgba").reshape(-1, 4)[built.name2id(2, "plain")].tolist() == [0.5, 0.5, 0.5, 1.0]
    outs = []
    for mm in (built, loaded):
        ee = ms.Engine(mm, NENV)
        outs.append(ee.render("cam", 30, 20) + ee.render("cam", 30, 20, ambient=1.0, diffuse=0.0)[3:])
        if mm is built:
            check_render("colour scene", *(x[0] for x in outs[0][:4]), rc.device_scene(ee, mm, 0), rc.camera_rays(ee, mm, 0, 0, 30, 20), rc.model_colours(mm))
        ee.close()
    assert same(outs[0], outs[1]), "colours set through the builder and through MJCF default classes and a material give the same images"
    assert len({tuple(c) for c in outs[0][4][0].reshape(-1, 4).tolist()}) >= 5, "floor, ball, crate, the grey capsule and the background are in view"


# ------------------------------------------------------------------ 9. the device form
def test_render_device_same_bits(prim):
    import torch
    m, e, scene = prim
    width, height, env0, n = 30, 20, 1, 3
    kw = dict(env0=env0, n=n, range=1, ambient=0.2, diffuse=0.9, background=(0.5, 0.25, 0.125, 1.0))
    ref = e.render("side", width, height, **kw)
    dev = torch.device("cuda:0")

    def buffers():
        return (torch.full((n, height, width), 7.0, dtype=torch.float32, device=dev), torch.full((n, height, width), 7, dtype=torch.int32, device=dev),
                torch.full((n, height, width, 3), 7.0, dtype=torch.float32, device=dev), torch.full((n, height, width, 4), 7, dtype=torch.uint8, device=dev))
    for take in ((1, 1, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (0, 0, 1, 1), (0, 1, 0, 1), (1, 0, 1, 0), (1, 1, 0, 0)):
        t = buffers()
        torch.cuda.synchronize()
        e.render_device(*(x.data_ptr() if k else None for x, k in zip(t, take)), "side", width, height, **kw)
        e.synchronize()
        for x, k, r in zip(t, take, ref):
            got = x.cpu().numpy()
            if k:
                assert np.array_equal(_bits(got), _bits(r)), take
            else:
                assert (got == 7).all(), (take, "an image the caller does not take is not written")
    d, g, nn, cc = e.render("side", width, height, normal=False, **kw)
    assert nn is None and same((d, g, cc), (ref[0], ref[1], ref[3]))
    d, g, nn, cc = e.render("side", width, height, rgba=False, **kw)
    assert cc is None and same((d, g, nn), ref[:3])
    o = capi.RenderOptions(); e.lib.mjh_render_default_options(C.byref(o))
    assert (o.view.camera, o.view.width, o.view.height, o.view.bodyexclude, o.view.flg_static, o.view.range, o.view.cull, o.view.cutoff) == (0, 64, 64, -1, 1, 0, 1, 0.0)
    assert (o.ambient, o.diffuse, list(o.background)) == (np.float32(0.3), np.float32(0.7), [0.0, 0.0, 0.0, 0.0])


# ------------------------------------------------------------------ 10. nothing of the state is written
def _snapshot(e):
    t, q, v, w = e.get_state()
    return [t, q, v, w, e.get_stats(), e.get_field("qacc"), e.get_field("qfrc_applied")]


def test_no_side_effects(lib):
    m = rc.prim_model(lib, gravity=(0, 0, -9.81))
    a, b = ms.Engine(m, NENV), ms.Engine(m, NENV)
    a.step(150); b.step(150)      # (the free bodies have begun to land on the floor)
    before = _snapshot(a)
    a.render("front", 30, 20); a.render("side", 9, 8, env0=1, n=2, cull=0, range=1, normal=False)
    for x, y in zip(before, _snapshot(a)):
        assert np.array_equal(x, y)
    a.step(3); b.step(3)
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "a step after a render call equals a step without one"
    a.step1(); out = a.render("front", 30, 20); a.step2()
    b.step1(); b.get_geom_state(0, NENV); b.step2()
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "the call sequence rules are those of mjh_get_geom_state"
    assert (out[1] >= 0).any()
    a.close(); b.close()


# ------------------------------------------------------------------ 11. errors
def test_errors_launch_nothing(prim, lib):
    m, e, scene = prim
    width, height = 9, 8
    good = e.render("front", width, height)
    bufs = [np.full((NENV, height, width), 7.0, np.float32), np.full((NENV, height, width), 7, np.int32),
            np.full((NENV, height, width, 3), 7.0, np.float32), np.full((NENV, height, width, 4), 7, np.uint8)]

    def call(eng=e, env0=0, n=NENV, null=False, ambient=None, diffuse=None, background=None, **kw):
        o = capi.RenderOptions(); lib.mjh_render_default_options(C.byref(o))
        o.view.width, o.view.height = width, height
        for k, v in kw.items():
            setattr(o.view, k, v)
        if ambient is not None: o.ambient = ambient
        if diffuse is not None: o.diffuse = diffuse
        if background is not None: o.background = (C.c_float * 4)(*background)
        return lib.mjh_render(eng.h, env0, n, C.byref(o), *(None if null else C.c_void_p(x.ctypes.data) for x in bufs))

    def ok():
        assert all((x == 7).all() for x in bufs), "nothing was launched: the outputs are untouched"
        assert call() == 0
        assert same(bufs, good)
        for x in bufs:
            x[...] = 7

    nan, inf = float("nan"), float("inf")
    for bad in (dict(camera=2), dict(camera=-1), dict(bodyexclude=m.nbody), dict(bodyexclude=-2), dict(width=0), dict(height=0), dict(width=-3),
                dict(env0=2, n=3), dict(env0=-1, n=2), dict(env0=NENV, n=1), dict(n=0), dict(null=True), dict(width=1 << 16, height=1 << 15),
                dict(ambient=-0.1), dict(ambient=nan), dict(ambient=inf), dict(diffuse=-1.0), dict(diffuse=nan), dict(diffuse=inf),
                dict(background=(0, 0, 1.5, 0)), dict(background=(-0.1, 0, 0, 0)), dict(background=(0, nan, 0, 0))):
        assert call(**bad) == MJH_ERR_ARG, bad
        assert lib.mjh_last_error()
        ok()
    assert lib.mjh_render_device(e.h, 0, NENV, None, None, None, None, None) == MJH_ERR_ARG
    ok()
    with pytest.raises(MjhError):
        e.render("front", 0, 8)
    with pytest.raises(ValueError):
        e.render("no such camera", 8, 8)
    with pytest.raises(TypeError):
        e.render("front", 8, 8, per_env=1)
    with pytest.raises(MjhError):
        e.render("front", 8, 8, ambient=-1.0)
    ok()
    s = ms.scene("s24"); es = ms.Engine(s, NENV)
    assert s.ncam == 0 and call(eng=es) == MJH_ERR_ARG and b"camera" in lib.mjh_last_error()
    assert all((x == 7).all() for x in bufs)
    es.step(2)      # (and the engine goes on as usual)
    es.close()
    ok()
