"""2D textures in the colour image on the device (mjh_render_set_texturing 1, csrc/texture.hip) against the fp64 reference
tests/texture_ref.py, by the comparison of tests/texture_check.py: on the pixels the reference finds robust, feature-robust,
light-stable (lit images) and texel-stable (at most 2 % of an image are left out, asserted) the flat image holds the texels' bytes
exactly, and a shaded or lit image is within the allowance that route has without textures; a miss is the background exactly.  The
reference works from the device's own poses (mjh_get_body_state, mjh_get_geom_state).  4 envs, images of at most 30 x 20 pixels.

`pytest tests/test_gpu_texture.py -m gpu -s` prints every case; DESIGN.md section 4e has what one MI355X gave."""
import ctypes as C

import numpy as np
import pytest

import light_check as lc
import mujoco_sim_amd as ms
import render_check as rc
import texture_check as tc
from mujoco_sim_amd import capi
from mujoco_sim_amd.engine import MjhError
from test_gpu_light import _bits, same, spread_free_bodies
from texture_check import NENV

pytestmark = pytest.mark.gpu

MJH_ERR_ARG = -1
LIGHTS = (lc.SPOT, lc.SUN)


def engine(m, texturing=1, lighting=0):
    e = ms.Engine(m, NENV)
    e.render_texturing = texturing
    e.render_lighting = lighting
    return e


@pytest.fixture(scope="module")
def white(lib):
    """every geom white: the flat image is the texel image"""
    m = tc.prim_model(lib)
    e = engine(m)
    spread_free_bodies(e, m)
    yield m, e
    e.close()


@pytest.fixture(scope="module")
def prim(lib):
    """palette colours, the two lights of light_check"""
    m = tc.prim_model(lib, coloured=True, lights=LIGHTS)
    e = engine(m)
    spread_free_bodies(e, m)
    yield m, e
    e.close()


def env_inputs(e, m, cam, width, height, env, size=None):
    return rc.device_scene(e, m, env, size=size), rc.camera_rays(e, m, m.name2id(5, cam), env, width, height)


# ------------------------------------------------------------------ 1. exact texels
@pytest.mark.parametrize("cam", ["front", "side"])
@pytest.mark.parametrize("width,height", [(30, 20), (8, 8), (9, 8), (1, 1)])
def test_exact_texels(white, cam, width, height):
    m, e = white
    textures, records = tc.prim_textures(), tc.model_records(m)
    assert all(np.array_equal(a, b) for a, b in zip(textures, tc.model_textures(m)))
    out = e.render(cam, width, height, ambient=1.0, diffuse=0.0)
    assert out[3].shape == (NENV, height, width, 4) and out[3].dtype == np.uint8
    seen = 0
    for env in (range(NENV) if (width, height) == (30, 20) else (0, NENV - 1)):
        scene, rays = env_inputs(e, m, cam, width, height, env)
        ntex, _, _ = tc.check_texels(f"exact {cam} {width}x{height} env {env}", out[1][env], out[3][env], scene, rays, textures, records)
        seen += ntex
    if (width, height) == (30, 20):
        assert seen >= 400, "the comparison sees textured pixels in every env"
        g = out[1][0].ravel(); c = out[3][0].reshape(-1, 4)
        for geom in (0, 5):      # the floor and the box show more than one texel
            assert len({tuple(x) for x in c[g == geom, :3]}) >= 2, geom


# ------------------------------------------------------------------ 2. shaded and lit
@pytest.mark.parametrize("lighting", [0, 1])
@pytest.mark.parametrize("cam,width,height", [("front", 30, 20), ("side", 30, 20), ("front", 9, 8), ("side", 8, 8), ("side", 1, 1)])
def test_shaded_and_lit(prim, lighting, cam, width, height):
    m, e = prim
    textures, records = tc.prim_textures(), tc.model_records(m)
    e.render_lighting = lighting
    out = e.render(cam, width, height, ambient=0.3, diffuse=0.7)
    e.render_lighting = 0
    for env in ((0, 1, NENV - 1) if (width, height) == (30, 20) else (0,)):
        scene, rays = env_inputs(e, m, cam, width, height, env)
        worst, ntex, _, _ = tc.check_colour(f"{'lit' if lighting else 'shaded'} {cam} {width}x{height} env {env}", out[1][env], out[3][env], scene, rays,
                                            rc.model_colours(m), textures, records, lights=lc.device_lights(e, m, env) if lighting else None)
        if (width, height) == (30, 20):
            assert ntex >= 100


# ------------------------------------------------------------------ 3. the texture follows the geom's frame
def test_a_moving_textured_body(white):
    m, e = white
    textures, records = tc.prim_textures(), tc.model_records(m)
    assert records[tc.FREE_BOX]["tex"] == 3 and m.array("body_weldid")[m.array("geom_bodyid")[tc.FREE_BOX]] != 0
    # every env its own pose and orientation of the free box
    rng = np.random.default_rng(7)
    q = np.tile(m.array("qpos0"), (NENV, 1))
    adr = int(m.array("jnt_qposadr")[m.array("body_jntadr")[m.array("geom_bodyid")[tc.FREE_BOX]]])
    for i in range(1, NENV):
        q[i, adr:adr + 3] += rng.uniform(-0.08, 0.08, size=3)
        quat = q[i, adr + 3:adr + 7] + rng.uniform(-0.3, 0.3, size=4); q[i, adr + 3:adr + 7] = quat / np.linalg.norm(quat)
    e.set_state(qpos=q, qvel=np.zeros((NENV, m.nv)))
    out = e.render("side", 30, 20, ambient=1.0, diffuse=0.0)
    box = []
    for env in range(NENV):
        scene, rays = env_inputs(e, m, "side", 30, 20, env)
        tc.check_texels(f"moving box env {env}", out[1][env], out[3][env], scene, rays, textures, records)
        box.append(out[3][env][out[1][env] == tc.FREE_BOX])
        assert len(box[-1]) >= 4, "the camera sees the free box"
    assert all(not np.array_equal(out[3][0], out[3][i]) for i in range(1, NENV)), "the envs' images differ"
    spread_free_bodies(e, m)      # (the fixture's poses again)


# ------------------------------------------------------------------ 4. a non-uniform texture takes the env's own size
def test_per_env_size(lib):
    m = tc.prim_model(lib)
    e = engine(m)
    textures, records = tc.prim_textures(), tc.model_records(m)
    size = m.array("geom_size")
    big = size.copy().reshape(-1, 3); big[5] = big[5] * [2.0, 2.0, 1.5]; big = big.ravel().astype(np.float32).astype(float)
    base = e.render("front", 30, 20, ambient=1.0, diffuse=0.0)
    e.set_env_param("geom_size", big[None, :], env0=2)
    out = e.render("front", 30, 20, ambient=1.0, diffuse=0.0)
    for env in range(NENV):
        scene, rays = env_inputs(e, m, "front", 30, 20, env, size=big if env == 2 else size)
        tc.check_texels(f"per-env size env {env}", out[1][env], out[3][env], scene, rays, textures, records)
    assert np.array_equal(out[3][0], base[3][0]) and not np.array_equal(out[3][2], base[3][2])
    # the reference with the model's size does not fit env 2: the half extents are the env's
    scene, rays = env_inputs(e, m, "front", 30, 20, 2, size=big)
    centre, _, t_new, has, keep, _, _ = tc.kept_pixels("env 2, its own size", scene, rays, textures, records)
    wrong = dict(scene, size=np.asarray(size, float).reshape(-1, 3))
    t_old, _ = tc.tr.texels(textures, records, wrong, centre[1], tc.tr.hit_points(rays, centre[0], centre[1]))
    on_box = keep & (centre[1] == 5)
    assert on_box.sum() >= 4 and (t_old[on_box] != t_new[on_box]).any(), "the case tells the two sizes apart"
    e.close()


# ------------------------------------------------------------------ 5. a textured height field
def test_hfield(lib):
    m = tc.hfield_model(lib)
    e = engine(m)
    textures, records = tc.hfield_textures(), tc.model_records(m)
    out = e.render("cam", 30, 20, ambient=1.0, diffuse=0.0)
    scene, rays = env_inputs(e, m, "cam", 30, 20, 0)
    # (the terrain is green: the flat image is level(rgba * t / 255), compared through the shaded route's reference)
    worst, ntex, _, _ = tc.check_colour("hfield", out[1][0], out[3][0], scene, rays, rc.model_colours(m), textures, records, ambient=1.0, diffuse=0.0, tol=1)
    assert ntex >= 100 and len({tuple(x) for x in out[3][0].reshape(-1, 4)[out[1][0].ravel() == 0, :3]}) >= 8, "many texels of the terrain's texture"
    e.close()


# ------------------------------------------------------------------ 6. untextured pixels are untouched; mode 0; no textures
@pytest.mark.parametrize("lighting", [0, 1])
def test_untextured_pixels_and_mode_0(lib, prim, lighting):
    m, e = prim
    records = tc.model_records(m)
    plain_model = tc.prim_model(lib, coloured=True, textured=False, lights=LIGHTS)
    assert plain_model.ntex == 0 and m.ntex == 4
    p = engine(plain_model, texturing=0, lighting=lighting)
    spread_free_bodies(p, plain_model)
    for cam, w, h in (("side", 30, 20), ("front", 9, 8)):
        ref0 = p.render(cam, w, h)
        p.render_texturing = 1
        assert same(p.render(cam, w, h), ref0), "texturing 1 on a model without textures is texturing 0"
        p.render_texturing = 0
        e.render_lighting = lighting
        e.render_texturing = 0
        off = e.render(cam, w, h)
        e.render_texturing = 1
        on = e.render(cam, w, h)
        e.render_lighting = 0
        assert same(off, ref0), "texturing 0 on the textured model equals the model built without textures"
        assert same(on[:3], off[:3]), "depth, geom id and normal are texturing 0's"
        textured = np.isin(on[1], [g for g, R in enumerate(records) if R["tex"] >= 0])
        assert np.array_equal(on[3][~textured], off[3][~textured]), "a pixel whose geom has no texture keeps its bytes"
        assert (on[3][textured] != off[3][textured]).any() and textured.any() and (~textured).any()
    p.close()


# ------------------------------------------------------------------ 7. the device form
@pytest.mark.parametrize("lighting", [0, 1])
def test_device_form_same_bits(prim, lighting):
    import torch
    m, e = prim
    e.render_lighting = lighting
    want = e.render("side", 30, 20)
    dev = torch.device("cuda:0")
    for take in ((1, 1, 1, 1), (0, 0, 0, 1), (1, 0, 0, 1), (1, 1, 1, 0)):
        t = (torch.full((NENV, 20, 30), 7.0, dtype=torch.float32, device=dev), torch.full((NENV, 20, 30), 7, dtype=torch.int32, device=dev),
             torch.full((NENV, 20, 30, 3), 7.0, dtype=torch.float32, device=dev), torch.full((NENV, 20, 30, 4), 7, dtype=torch.uint8, device=dev))
        torch.cuda.synchronize()
        e.render_device(*(x.data_ptr() if k else None for x, k in zip(t, take)), "side", 30, 20)
        e.synchronize()
        for x, k, r in zip(t, take, want):
            got = x.cpu().numpy()
            assert np.array_equal(_bits(got), _bits(r)) if k else (got == 7).all(), take
    d, g, nn, cc = e.render("side", 30, 20, normal=False)
    assert nn is None and same((d, g, cc), (want[0], want[1], want[3]))
    part = e.render("side", 30, 20, env0=1, n=2)
    assert same(part, tuple(x[1:3] for x in want)), "a range of envs gives those envs' images"
    e.render_lighting = 0


# ------------------------------------------------------------------ 8. more than 64 geoms: two staging passes of the depth launch
def test_many_spheres_two_passes(lib):
    m = tc.spheres_model(lib)
    assert m.ngeom > 64
    e = engine(m)
    textures, records = tc.spheres_textures(), tc.model_records(m)
    out = e.render("above", 16, 16)
    scene, rays = env_inputs(e, m, "above", 16, 16, 0)
    worst, ntex, _, _ = tc.check_colour("many spheres", out[1][0], out[3][0], scene, rays, rc.model_colours(m), textures, records)
    assert ntex >= 100 and all((out[1][0] == g).any() and records[g]["tex"] == 1 for g in tc.SECOND_PASS), "the floor and textured spheres of the second pass are seen"
    for env in range(1, NENV):
        assert np.array_equal(out[3][env], out[3][0])
    e.close()


# ------------------------------------------------------------------ 9. errors launch nothing
def test_errors_launch_nothing(prim, lib):
    m, e = prim
    width, height = 9, 8
    good = e.render("front", width, height)
    bufs = [np.full((NENV, height, width), 7.0, np.float32), np.full((NENV, height, width), 7, np.int32),
            np.full((NENV, height, width, 3), 7.0, np.float32), np.full((NENV, height, width, 4), 7, np.uint8)]

    def call():
        o = capi.RenderOptions(); lib.mjh_render_default_options(C.byref(o))
        o.view.width, o.view.height = width, height
        return lib.mjh_render(e.h, 0, NENV, C.byref(o), *(C.c_void_p(x.ctypes.data) for x in bufs))

    for mode in (2, -1, 7):
        assert lib.mjh_render_set_texturing(e.h, mode) == MJH_ERR_ARG and lib.mjh_last_error()
        assert all((x == 7).all() for x in bufs), "nothing was launched: the outputs are untouched"
        assert e.render_texturing == 1
        assert call() == 0 and same(bufs, good), "a following render equals the earlier one"
        for x in bufs:
            x[...] = 7
    with pytest.raises(MjhError):
        e.render_texturing = 3
    assert lib.mjh_render_set_texturing(None, 1) == MJH_ERR_ARG and lib.mjh_render_get_texturing(None) == 0
    s = ms.scene("s24"); es = ms.Engine(s, NENV)
    assert es.render_texturing == 0 and lib.mjh_render_set_texturing(es.h, 1) == 0
    es.step(2)
    es.close()
