"""Lights and cast shadows in the colour image on the device (mjh_render_set_lighting 1, csrc/light.hip) against the fp64 reference
tests/light_ref.py, by the comparison of tests/light_check.py: on the pixels the reference finds robust, feature-robust and light-stable
(at most 2 % of an image are left out, asserted) every colour channel is within 2 + ceil(255 K sqrt(3) TOL_N) levels; a miss is the
background exactly.  The reference works from the device's own poses (mjh_get_body_state, mjh_get_geom_state).  4 envs, images of at
most 30 x 20 pixels.

Measured on one MI355X (`pytest tests/test_gpu_light.py -m gpu -s` prints every case): colour difference 0 levels in all 42 compared
images (allowed 3); largest excluded share 1.56 % (side view 8 x 8: one pixel of 64), then 0.33 %; DESIGN.md section 4d has the
cast-shadow pixel counts."""
import ctypes as C

import numpy as np
import pytest

import light_check as lc
import light_ref as lr
import mujoco_sim_amd as ms
import ray_mesh_ref as rm
import ray_ref as rr
import render_check as rc
import render_ref as rf
from helpers import set_opt
from light_check import NENV, check_light
from mujoco_sim_amd import capi
from mujoco_sim_amd.engine import MjhError

pytestmark = pytest.mark.gpu

MJH_ERR_ARG = -1


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32) if a.dtype == np.float32 else np.ascontiguousarray(a)


def same(a, b):
    return all((x is None and y is None) or np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def engine(m, lighting=1):
    e = ms.Engine(m, NENV)
    e.render_lighting = lighting
    return e


def spread_free_bodies(e, m, seed=31, amount=0.05):
    """every env but env 0 gets its own pose of every free body (gravity is off: the poses stay)"""
    rng = np.random.default_rng(seed)
    q = np.tile(m.array("qpos0"), (NENV, 1))
    for j in np.nonzero(m.array("jnt_type") == 0)[0]:
        a = int(m.array("jnt_qposadr")[j])
        q[1:, a:a + 3] += rng.uniform(-amount, amount, size=(NENV - 1, 3))
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv)))


@pytest.fixture(scope="module")
def prim(lib):
    m = lc.prim_model(lib)
    e = engine(m)
    spread_free_bodies(e, m)
    yield m, e
    e.close()


def check_env(name, e, m, cam, width, height, env, out, surface=None, size=None, visible=None, active=None, **kw):
    rays = rc.camera_rays(e, m, m.name2id(5, cam), env, width, height)
    scene = rc.device_scene(e, m, env, size=size, visible=visible, surface=surface)
    return check_light(f"{name} env {env}", out[1][env], out[3][env], scene, rays, rc.model_colours(m), lc.device_lights(e, m, env, active), **kw)


# ------------------------------------------------------------------ 1. the primitives scene under two lights: tile edges, a pose per env
@pytest.mark.parametrize("cam", ["front", "side"])
@pytest.mark.parametrize("width,height", [(30, 20), (8, 8), (9, 8), (1, 1)])
def test_primitives_two_lights(prim, cam, width, height):
    m, e = prim
    out = e.render(cam, width, height)
    assert out[3].shape == (NENV, height, width, 4) and out[3].dtype == np.uint8
    for env in (range(NENV) if (width, height) == (30, 20) else (0, NENV - 1)):
        worst, share, shadowed = check_env(f"primitives {cam} {width}x{height}", e, m, cam, width, height, env, out)
        if (width, height) == (30, 20):
            assert min(shadowed) >= 8, "both lights cast shadows the comparison sees: an unshadowed image cannot pass"
    if (width, height) == (30, 20):
        assert not np.array_equal(out[3][0], out[3][1]), "every env has its own image"
        e.render_lighting = 0
        plain = e.render(cam, width, height)
        e.render_lighting = 1
        assert same(plain[:3], out[:3]) and not np.array_equal(plain[3], out[3])


# ------------------------------------------------------------------ 2. a positional light inside the scene: the bound x < 1, a narrow cone
def test_positional_light_below_some_geoms(lib):
    m = lc.prim_model(lib, lights=(lc.LOW_SPOT,))
    e = engine(m)
    shadowed = beyond = lit_px = 0
    for cam in ("front", "side"):
        out = e.render(cam, 30, 20)
        _, _, s = check_env(f"low spot {cam}", e, m, cam, 30, 20, 0, out)
        shadowed += s[0]
        # lit pixels whose shadow ray, continued past the light, meets a geom: only the bound keeps them lit
        rays = rc.camera_rays(e, m, m.name2id(5, cam), 0, 30, 20)
        scene = rc.device_scene(e, m, 0)
        L = lc.device_lights(e, m, 0)
        centre, term, cast, keep, _ = lc.kept_pixels(f"low spot {cam}", scene, rays, L)
        d, g, n, _ = centre
        lit = keep & (term[0][:, 0] > 0.05)
        o = rays[0] + np.where(g >= 0, d, 0.0)[:, None] * rays[1] + lc.BIAS * n
        sd, sg = rm.cast(o[lit], L[0]["pos"] - o[lit], scene)
        beyond += int(((sg >= 0) & (sd >= 1)).sum()); lit_px += int(lit.sum())
    print(f"low spot: {shadowed} kept cast-shadow pixels, {lit_px} lit, {beyond} of them with a geom beyond the light")
    assert shadowed >= 2 and beyond >= 4 and lit_px >= 20
    e.close()


# ------------------------------------------------------------------ 3. a light on a free body: a light pose per env
RIG_LIGHT = dict(name=b"riglight", pos=(0.0, 0.0, -0.3), dir=(0.0, 0.0, -1.0), directional=0, castshadow=1, diffuse=(0.8, 0.7, 0.6), ambient=(0.0, 0.0, 0.05),
                 cutoff=45.0, exponent=2.0)


def test_light_on_a_free_body(lib):
    m = lc.prim_model(lib, lights=(), rig=True, light_on_rig=RIG_LIGHT)
    e = engine(m)
    rng = np.random.default_rng(29)
    bd = m.name2id(0, "rig")
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[bd]])
    q = np.tile(m.array("qpos0"), (NENV, 1))
    for i in range(NENV):
        q[i, adr:adr + 3] = [rng.uniform(-1.2, 1.2), rng.uniform(-0.6, 0.6), rng.uniform(2.6, 3.2)]
        tilt = rng.uniform(-0.25, 0.25, size=3)
        quat = np.array([1.0, *(0.5 * tilt)]); q[i, adr + 3:adr + 7] = quat / np.linalg.norm(quat)
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv)))
    out = e.render("front", 30, 20)
    poses = []
    for env in range(NENV):
        _, _, s = check_env("rig light", e, m, "front", 30, 20, env, out)
        L = lc.device_lights(e, m, env)
        poses.append(np.concatenate([L[0]["pos"], L[0]["dir"]]))
        assert s[0] >= 4, "the hovering geoms shadow the floor under the carried light"
    assert min(np.abs(poses[i] - poses[j]).max() for i in range(NENV) for j in range(i)) > 0.05, "the envs' light poses differ"
    assert not np.array_equal(out[3][0], out[3][1])
    e.close()


# ------------------------------------------------------------------ 4. 70 spheres under a low sun: two staging passes, occluders in both
def test_many_spheres_two_passes(lib):
    m = lc.spheres_model(lib)
    assert m.ngeom > 64
    e = engine(m)
    out = e.render("above", 16, 16)
    _, _, s = check_env("many spheres", e, m, "above", 16, 16, 0, out)
    assert s[0] >= 8
    rays = rc.camera_rays(e, m, 0, 0, 16, 16); scene = rc.device_scene(e, m, 0); L = lc.device_lights(e, m, 0)
    centre, term, cast, keep, _ = lc.kept_pixels("many spheres", scene, rays, L)
    d, g, n, _ = centre
    k = cast[0] & keep
    o = rays[0] + d[:, None] * rays[1] + lc.BIAS * n
    _, sg = rm.cast(o[k], np.tile(-L[0]["dir"], (int(k.sum()), 1)), scene)
    print(f"many spheres: occluders of the first pass {int((sg < 64).sum())}, of the second {int((sg >= 64).sum())}")
    assert (sg >= 64).any() and ((sg >= 0) & (sg < 64)).any(), "the nearest occluder lies in either staging pass"
    for env in range(1, NENV):
        assert np.array_equal(out[3][env], out[3][0])
    e.close()


EDGE_SUN = {65: (0.1, 1.0, -0.3), 130: (0.1, 1.0, -0.4)}      # low suns under which shadow rays meet geoms of the first and of the last pass


def edge_occluders(spec, rays, L, centre, cast, keep):
    """per light: (a kept cast-shadow pixel whose shadow ray a geom of the FIRST staging pass blocks, one that only geoms of the LAST
    pass block), from the fp64 reference cast against the geoms of one pass at a time"""
    d, g, n, _ = centre
    npass = (len(spec) + 63) // 64
    out = []
    for l in range(len(L)):
        k = cast[l] & keep
        o = rays[0][k] + d[k, None] * rays[1][k] + lc.BIAS * n[k]
        v = np.tile(-np.asarray(L[l]["dir"]), (int(k.sum()), 1))
        hit = np.array([rm.cast(o, v, rr.scene_from_spec(spec[64 * p:64 * (p + 1)]))[1] >= 0 for p in range(npass)])
        out.append((bool(hit[0].any()), bool((hit[-1] & ~hit[:-1].any(axis=0)).any())))
    return out


@pytest.mark.parametrize("ngeom", [65, 130])
def test_staging_pass_edges(lib, ngeom):
    """65 geoms: the second staging pass holds a single candidate; 130: a third pass follows a full second one.  A low sun over the
    last sphere, 9 x 8 pixels (tiles partial in both directions): some shadow rays are blocked by a geom of the first pass (those lanes
    stop walking there), some only by a geom of the last one, and the lit pixels walk every pass.  NOT pinned here: that a whole wave leaves
    the pass loop through the wave-uniform `break` (`__ballot(walking) == 0`) before the last pass — that takes a tile whose every walking
    lane is blocked early, which these 72 pixels do not guarantee"""
    spec, last = rr.pass_edge_spec(ngeom)
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    rc.add_spec(lib, b, spec, rc.palette(len(spec), seed=6))
    rc.add_camera(lib, b, b"over", 0, ((last[0] + 0.3, last[1] - 0.8, 3.0), (last[0] - 0.25, last[1] - 0.15, 0.5), 45.0))
    lc.add_light(lib, b, 0, dict(lc.LOW_SUN, dir=EDGE_SUN[ngeom]))
    m = rc.compile_model(lib, b)
    assert m.ngeom == ngeom and m.nlight == 1
    e = engine(m)
    out = e.render("over", 9, 8)
    e.light_options = dict(cull=0)
    assert same(e.render("over", 9, 8), out), "cull 0 and 1 give equal bytes"
    e.light_options = dict(cull=1)
    for env in range(1, NENV):
        assert np.array_equal(out[3][env], out[3][0])
    check_env(f"{ngeom} geoms 9x8", e, m, "over", 9, 8, 0, out)
    rays = rc.camera_rays(e, m, 0, 0, 9, 8); L = lc.device_lights(e, m, 0)
    centre, term, cast, keep, _ = lc.kept_pixels(f"{ngeom} geoms 9x8", rc.device_scene(e, m, 0), rays, L)
    occ = edge_occluders(spec, rays, L, centre, cast, keep)
    print(f"{ngeom} geoms: per light (blocked by the first pass, blocked by the last pass alone) {occ}")
    assert occ[0] == (True, True)
    lit = keep & (centre[1] >= 0) & ~cast[0] & (term.max(axis=(0, 2)) > 0.05)
    assert lit.sum() >= 8, "lit pixels: their lanes walk every pass"
    e.close()


# ------------------------------------------------------------------ 5. the height field shadows itself; meshes as hulls and as triangles
def test_hfield_self_shadow(lib):
    m = lc.hfield_model(lib)
    e = engine(m)
    out = e.render("cam", 30, 20)
    _, _, s = check_env("hfield", e, m, "cam", 30, 20, 0, out)
    rays = rc.camera_rays(e, m, 0, 0, 30, 20)
    centre, term, cast, keep, _ = lc.kept_pixels("hfield", rc.device_scene(e, m, 0), rays, lc.device_lights(e, m, 0))
    assert ((centre[1] == 0) & cast[0] & keep).sum() >= 8, "terrain pixels in the terrain's own shadow"
    e.close()


def test_mesh_hulls_and_triangles(lib):
    m, (g_torus, g_jaw, g_quad) = lc.meshes_model(lib)
    e = engine(m)
    width, height = 24, 16
    e.ray_mesh_mode = 1
    hull = e.render("cam", width, height)
    check_env("meshes, hulls", e, m, "cam", width, height, 0, hull, surface=0)
    e.ray_mesh_surface = 1
    tri = e.render("cam", width, height)
    check_env("meshes, triangles", e, m, "cam", width, height, 0, tri, surface=1)
    rays = rc.camera_rays(e, m, 0, 0, width, height); L = lc.device_lights(e, m, 0)
    ref = {s: lc.kept_pixels(f"meshes surface {s}", rc.device_scene(e, m, 0, surface=s), rays, L) for s in (0, 1)}
    through = (ref[0][0][1] == 0) & (ref[1][0][1] == 0) & ref[0][3] & ref[1][3] & ref[0][2][0] & ~ref[1][2][0]
    assert through.sum() >= 2, "the hull fills the torus's hole; the triangles let the light through"
    h, t = hull[3][0].reshape(-1, 4).astype(int), tri[3][0].reshape(-1, 4).astype(int)
    assert (t[through, :3].sum(axis=1) > h[through, :3].sum(axis=1) + 30).all(), "there the floor is lit under the triangles and dark under the hulls"
    e.close()


# ------------------------------------------------------------------ 6. the camera inside its ball: every light outside gives its ambient term only
def test_camera_inside_its_ball(lib):
    m = lc.prim_model(lib, rig=True)
    e = engine(m)
    out = e.render("eye", 30, 20)
    rigg = m.name2id(2, "rigg")
    assert (out[1] == rigg).all()
    check_env("inside the ball", e, m, "eye", 30, 20, 0, out)
    rays = rc.camera_rays(e, m, 2, 0, 30, 20); L = lc.device_lights(e, m, 0)
    term, _ = lr.terms(L, rays, rc.device_scene(e, m, 0))
    assert all(np.array_equal(term[k], np.tile(L[k]["ambient"], (600, 1))) for k in range(2)), "the reference: a light outside the ball is blocked by it"
    e.light_options = dict(shadows=0)
    assert not np.array_equal(e.render("eye", 30, 20)[3], out[3]), "without shadow rays the lights shine through the ball"
    e.close()


# ------------------------------------------------------------------ 7. visibility: what the camera ray cannot see casts no shadow
def test_visibility(lib):
    m = lc.prim_model(lib)
    e = engine(m)
    body = m.array("geom_bodyid")
    size = m.array("geom_size")
    base = e.render("front", 30, 20)
    rays = rc.camera_rays(e, m, 0, 0, 30, 20); L = lc.device_lights(e, m, 0)
    # the free body whose geom blocks the sun for the most kept pixels
    scene = rc.device_scene(e, m, 0)
    full = lc.kept_pixels("all visible", scene, rays, L)
    def freed(b):      # floor pixels in cast shadow with everything visible that are lit once body b is hidden
        h = lc.kept_pixels(f"body {b} hidden", rc.device_scene(e, m, 0, visible=body != b), rays, L)
        return int(((full[0][1] == 0) & (h[0][1] == 0) & full[3] & h[3] & full[2].any(axis=0) & ~h[2].any(axis=0)).sum())
    counts = {b: freed(b) for b in range(1, m.nbody) if (body == b).any()}
    bd = max(counts, key=counts.get)
    print(f"floor pixels a hidden body gives back to the light: {counts}")
    assert counts[bd] >= 2, "hiding that body removes shadow pixels"
    out = e.render("front", 30, 20, bodyexclude=bd)
    check_env("bodyexclude", e, m, "front", 30, 20, 0, out, visible=body != bd)
    static = m.array("body_weldid")[body] == 0
    out = e.render("front", 30, 20, flg_static=0)
    check_env("flg_static 0", e, m, "front", 30, 20, 0, out, visible=~static)
    # far plane: pixels beyond it are misses; the shadow rays are not bounded by it
    # (the floor's depth is constant along an image row: the plane is put into the widest gap between depths of the middle half)
    ds = np.sort(full[0][0][full[0][0] >= 0]); q = len(ds) // 4
    i = q + int(np.argmax(np.diff(ds[q:3 * q])))
    cut = float(0.5 * (ds[i] + ds[i + 1]))
    out = e.render("front", 30, 20, cutoff=cut, background=(0.1, 0.2, 0.3, 1.0))
    check_env("cutoff", e, m, "front", 30, 20, 0, out, cutoff=cut, background=(0.1, 0.2, 0.3, 1.0))
    assert (out[1][0] < 0).sum() > (base[1][0] < 0).sum()
    # an inactive slot in env 2, smaller geoms in env 1
    small = (0.8 * size).astype(np.float32).astype(float)
    e.set_env_param("geom_size", small[None, :], env0=1)
    e.set_slot_active(bd, 0, env0=2, n=1)
    out = e.render("front", 30, 20)
    for env in range(NENV):
        check_env("per-env sizes / slot", e, m, "front", 30, 20, env, out, size=small if env == 1 else size, visible=(body != bd) if env == 2 else None)
    assert same(tuple(x[0] for x in out), tuple(x[0] for x in base)) and same(tuple(x[3] for x in out), tuple(x[3] for x in base))
    assert not np.array_equal(out[3][1], base[3][1]) and not np.array_equal(out[3][2], base[3][2]), "smaller geoms and a hidden body change the shadows"
    e.close()


# ------------------------------------------------------------------ 8. exactness
def test_exactness(lib, prim):
    m, e = prim
    plainm = rc.prim_model(lib)
    assert plainm.nlight == 0 and m.nlight == 2
    p = ms.Engine(plainm, NENV)
    spread_free_bodies(p, plainm)
    ref0 = p.render("side", 30, 20)
    p.render_lighting = 1
    assert same(p.render("side", 30, 20), ref0), "mode 1 on a model without lights is mode 0"
    p.close()
    lit = e.render("side", 30, 20)
    e.render_lighting = 0
    assert e.render_lighting == 0 and same(e.render("side", 30, 20), ref0), "mode 0 on a model with lights equals the model without lights"
    e.render_lighting = 1
    assert same(lit[:3], ref0[:3]) and not np.array_equal(lit[3], ref0[3]), "depth, geom id and normal are mode 0's; the colour is not"
    for l in (0, 1):
        e.set_light_active(l, False)
    assert same(e.render("side", 30, 20), ref0), "mode 1 with every light inactive equals mode 0"
    e.set_light_active("sun", True)
    one = e.render("side", 30, 20)
    check_env("only the sun", e, m, "side", 30, 20, 1, one, active=[0, 1])
    e.set_light_active(0, True)
    assert same(e.render("side", 30, 20), lit)
    # shadows off: the reference without shadow rays; cull off: the same bytes
    e.light_options = dict(shadows=0)
    ns = e.render("side", 30, 20)
    check_env("no shadows", e, m, "side", 30, 20, 2, ns, shadows=False)
    assert not np.array_equal(ns[3], lit[3])
    e.light_options = dict(shadows=1, cull=0)
    assert e.light_options == dict(shadows=1, cull=0, bias=np.float32(1e-3))
    for cam, w, h in (("side", 30, 20), ("front", 9, 8)):
        off = e.render(cam, w, h)
        e.light_options = dict(cull=1)
        assert same(e.render(cam, w, h), off), "cull 0 and 1 give equal bytes"
        e.light_options = dict(cull=0)
    e.light_options = dict(cull=1)
    # another bias is another image, and the reference follows it
    e.light_options = dict(bias=5e-3)
    check_env("bias 5e-3", e, m, "side", 30, 20, 0, e.render("side", 30, 20), bias=5e-3)
    e.light_options = dict(bias=1e-3)


def test_device_form_same_bits(prim):
    """the device form equals the host form, with and without the caller's normal image (engine-owned scratch holds it then)"""
    import torch
    m, e = prim
    lit = e.render("side", 30, 20)
    dev = torch.device("cuda:0")
    for take in ((1, 1, 1, 1), (0, 0, 0, 1), (1, 0, 0, 1), (1, 1, 1, 0)):
        t = (torch.full((NENV, 20, 30), 7.0, dtype=torch.float32, device=dev), torch.full((NENV, 20, 30), 7, dtype=torch.int32, device=dev),
             torch.full((NENV, 20, 30, 3), 7.0, dtype=torch.float32, device=dev), torch.full((NENV, 20, 30, 4), 7, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        e.render_device(*(x.data_ptr() if k else None for x, k in zip(t, take)), "side", 30, 20)
        e.synchronize()
        for x, k, r in zip(t, take, lit):
            got = x.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(r)) if k else (got == 7).all(), take
    d, g, nn, cc = e.render("side", 30, 20, normal=False)
    assert nn is None and same((d, g, cc), (lit[0], lit[1], lit[3]))


def test_eight_lights_at_once(lib):
    rng = np.random.default_rng(11)
    lights = []
    for k in range(8):
        d = (float(rng.uniform(-0.6, 0.6)), float(rng.uniform(-0.6, 0.6)), -1.0)
        lights.append(dict(name=b"l%d" % k, pos=(float(rng.uniform(-2, 2)), float(rng.uniform(-1, 1)), 4.0 + 0.2 * k), dir=d, directional=k % 2, castshadow=1,
                           diffuse=(0.2, 0.15, 0.1), ambient=(0.01, 0.0, 0.0), cutoff=50.0, exponent=3.0))
    m = lc.prim_model(lib, lights=tuple(lights))
    assert m.nlight == 8
    e = engine(m)
    out = e.render("front", 8, 8)
    _, _, s = check_env("eight lights", e, m, "front", 8, 8, 0, out)
    print(f"eight lights: kept cast-shadow pixels per light {s}")
    assert all(x > 0 for x in s), "every one of the eight lights casts a shadow the comparison sees"
    e.close()


# ------------------------------------------------------------------ 9. no side effects; errors launch and write nothing
def _snapshot(e):
    t, q, v, w = e.get_state()
    return [t, q, v, w, e.get_stats(), e.get_field("qacc"), e.get_field("qfrc_applied")]


def test_no_side_effects(lib):
    m = lc.prim_model(lib, gravity=(0, 0, -9.81))
    a, b = engine(m), ms.Engine(m, NENV)
    a.step(150); b.step(150)
    before = _snapshot(a)
    a.render("front", 30, 20); a.render("side", 9, 8, env0=1, n=2, normal=False)
    for x, y in zip(before, _snapshot(a)):
        assert np.array_equal(x, y)
    a.step(3); b.step(3)
    for x, y in zip(_snapshot(a), _snapshot(b)):
        assert np.array_equal(x, y), "a step after a lit render call equals a step without one"
    a.close(); b.close()


def test_errors_launch_nothing(prim, lib):
    m, e = prim
    width, height = 9, 8
    good = e.render("front", width, height)
    bufs = [np.full((NENV, height, width), 7.0, np.float32), np.full((NENV, height, width), 7, np.int32),
            np.full((NENV, height, width, 3), 7.0, np.float32), np.full((NENV, height, width, 4), 7, np.uint8)]

    def call(env0=0, n=NENV, **kw):
        o = capi.RenderOptions(); lib.mjh_render_default_options(C.byref(o))
        o.view.width, o.view.height = width, height
        for k, v in kw.items():
            setattr(o.view, k, v)
        return lib.mjh_render(e.h, env0, n, C.byref(o), *(C.c_void_p(x.ctypes.data) for x in bufs))

    def ok():
        assert all((x == 7).all() for x in bufs), "nothing was launched: the outputs are untouched"
        assert e.render_lighting == 1 and e.light_options == dict(shadows=1, cull=1, bias=np.float32(1e-3))
        assert call() == 0 and same(bufs, good)
        for x in bufs:
            x[...] = 7

    for mode in (2, -1, 7):
        assert lib.mjh_render_set_lighting(e.h, mode) == MJH_ERR_ARG and lib.mjh_last_error()
        ok()
    for bad in (dict(bias=0.0), dict(bias=-1e-3), dict(bias=float("nan")), dict(bias=float("inf")), dict(shadows=2), dict(cull=-1)):
        o = capi.LightOptions(1, 1, 1e-3)
        for k, v in bad.items():
            setattr(o, k, v)
        assert lib.mjh_render_set_light_options(e.h, C.byref(o)) == MJH_ERR_ARG, bad
        ok()
    assert lib.mjh_render_set_light_options(e.h, None) == MJH_ERR_ARG
    for light in (-1, 2, 8):
        assert lib.mjh_set_light_active(e.h, light, 0) == MJH_ERR_ARG
        ok()
    for bad in (dict(camera=2), dict(bodyexclude=m.nbody), dict(width=0), dict(env0=2, n=3), dict(n=0)):
        assert call(**bad) == MJH_ERR_ARG, bad
        ok()
    with pytest.raises(MjhError):
        e.render_lighting = 3
    with pytest.raises(TypeError):
        e.light_options = dict(soft=1)
    o = capi.LightOptions(); lib.mjh_light_default_options(C.byref(o))
    assert (o.shadows, o.cull, o.bias) == (1, 1, np.float32(1e-3))
    s = ms.scene("s24"); es = ms.Engine(s, NENV)
    assert lib.mjh_set_light_active(es.h, 0, 1) == MJH_ERR_ARG and lib.mjh_render_set_lighting(es.h, 1) == 0
    es.step(2)
    es.close()
    ok()
