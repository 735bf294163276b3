"""What tests/test_light_host.py (the light kernel's code on the CPU) and tests/test_gpu_light.py (mjh_render with lighting mode 1 on
the device) share: the lit models, and the comparison of ONE env's colour image with tests/light_ref.py.

The comparison.  A pixel is KEPT where render_check.kept_pixels keeps it AND the reference's per-light terms amb_l + dif_l t_l move by
at most TERM_TOL = 1e-3 under the four 1e-4 ray shifts of render_ref.shifted and under bias x 0.5 and bias x 2 (a pixel on a shadow's
edge, on a cone's edge, or one whose shadow ray grazes its own surface is left out).  The share left out is asserted to be at most
ray_check.CAP = 0.02.  On every kept hit each colour channel is within

    2 + ceil(255 K sqrt(3) TOL_N)  levels,  K = diffuse + sum_l max_c dif_l over the active lights:

one rounding step; one level for the hit point's error (TOL d / |L - h| through l^ and spot: below 0.05 level in these scenes); and
TOL_N = render_check.TOL_N through n . v^ and every n . l^.  With K <= 2.5 that is 3 levels.  A miss is the background exactly, alpha is 255.

C_HOST is the worst colour difference over the kept pixels of every image of tests/test_light_host.py (the host build of
csrc/dev_light.h against this reference).  Measured there: 0 levels in every image, with and without shadow rays; C_HOST = 1 leaves the
host build one rounding step.  On one MI355X (tests/test_gpu_light.py): 0 levels in all 42 compared images.

Excluded shares measured on the CPU (the same test; share / kept cast-shadow pixels per light): primitives under SPOT and SUN, front
30 x 20 0 / 11, 8; 8 x 8 0 / 3, 2; 9 x 8 0 / 4, 1; 1 x 1 0 / 0, 0; 64 x 48 0.0007 / 83, 51; side 30 x 20 0.0017 / 26, 23; 8 x 8 0.0156 (one
pixel of 64) / 3, 4; 9 x 8 0 / 3, 4; 1 x 1 0 / 0, 0; 64 x 48 0.0020 / 151, 150; LOW_SPOT front 0 / 0, side 0.0017 / 0 at qpos0 (4 on the
device's poses, 20 lit pixels with a geom beyond the light); 70 spheres under LOW_SUN 0 / 37; the height field under HF_SUN 0.0017 / 21;
meshes under MESH_SUN, hulls 0 / 16, triangles 0 / 17."""
import math

import numpy as np

import light_ref as lr
import ray_ref as rr
import ray_tri_ref as rt
import render_check as rc
import render_ref as rf
from helpers import D, set_opt
from ray_check import CAP

TERM_TOL = 1e-3
C_HOST = 1          # levels: worst host-build colour difference over every image of test_light_host.py
BIAS = 1e-3
NENV = rc.NENV

# the two lights of the primitives scene: a spot above the scene pointing down, a directional light from the side
SPOT = dict(name=b"spot", pos=(0.4, -0.6, 5.0), dir=(0.0, 0.0, -1.0), directional=0, castshadow=1, diffuse=(0.6, 0.5, 0.4), ambient=(0.05, 0.05, 0.1),
            cutoff=45.0, exponent=10.0)
SUN = dict(name=b"sun", pos=(0.0, 0.0, 0.0), dir=(0.5, 0.3, -1.0), directional=1, castshadow=1, diffuse=(0.3, 0.35, 0.4), ambient=(0.0, 0.0, 0.0),
           cutoff=45.0, exponent=10.0)
# a positional light INSIDE the scene's 0.5 .. 1.5 m band: geoms beyond it block nothing (the bound x < 1); a narrow cone
LOW_SPOT = dict(name=b"low", pos=(0.84, 0.45, 1.0), dir=(0.37, -0.27, -1.0), directional=0, castshadow=1, diffuse=(0.7, 0.7, 0.6), ambient=(0.0, 0.02, 0.0),
                cutoff=30.0, exponent=2.0)
LOW_SUN = dict(name=b"lowsun", pos=(0.0, 0.0, 0.0), dir=(1.0, 0.4, -0.45), directional=1, castshadow=1, diffuse=(0.6, 0.6, 0.5), ambient=(0.02, 0.02, 0.02),
               cutoff=45.0, exponent=10.0)
# a low sun against the terrain's slopes: the height field shadows itself (non-convex)
HF_SUN = dict(name=b"hfsun", pos=(0.0, 0.0, 0.0), dir=(-1.0, 0.3, -0.35), directional=1, castshadow=1, diffuse=(0.6, 0.6, 0.5), ambient=(0.02, 0.02, 0.02),
              cutoff=45.0, exponent=10.0)
# tilted against the camera above the meshes: the light through the torus's hole lands on floor the camera sees beside the torus
MESH_SUN = dict(name=b"meshsun", pos=(0.0, 0.0, 0.0), dir=(0.25, -0.3, -1.0), directional=1, castshadow=1, diffuse=(0.6, 0.6, 0.6), ambient=(0.0, 0.0, 0.0),
                cutoff=45.0, exponent=10.0)


def add_light(lib, b, body, L):
    lid = lib.mjh_builder_add_light(b, L["name"], body, D(*L["pos"]), D(*L["dir"]), L["directional"], L["castshadow"], D(*L["diffuse"]), D(*L["ambient"]),
                                    L["cutoff"], L["exponent"])
    assert lid >= 0, lib.mjh_last_error()
    return lid


# ------------------------------------------------------------------ models: render_check's scenes, with lights
def prim_model(lib, lights=(SPOT, SUN), gravity=(0, 0, 0), rig=False, light_on_rig=None):
    """render_check.prim_model's scene with lights on the world body; rig: the free ball with the camera inside; light_on_rig: one more
    light carried by that body"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=list(gravity))
    spec = rr.primitives_spec()
    rc.add_spec(lib, b, spec, rc.palette(len(spec)))
    rc.add_camera(lib, b, b"front", 0, rc.VIEW_FRONT)
    rc.add_camera(lib, b, b"side", 0, rc.VIEW_SIDE)
    if rig:
        bd = lib.mjh_builder_add_body(b, b"rig", 0, D(0.0, -3.5, 2.5), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        g = lib.mjh_builder_add_geom(b, b"rigg", bd, rr.SPHERE, D(rc.RIG_RADIUS, 0, 0), None, None, None, -1, -1, -1, -1)
        assert g >= 0 and lib.mjh_builder_set_geom_rgba(b, g, D(0.9, 0.4, 0.1, 1.0)) == 0
        assert lib.mjh_builder_add_camera(b, b"eye", bd, D(*rc.RIG_CAM_POS), D(*rc.RIG_CAM_QUAT), 60.0) == 2
        if light_on_rig is not None:
            add_light(lib, b, bd, light_on_rig)
    for L in lights:
        add_light(lib, b, 0, L)
    return rc.compile_model(lib, b)


def spheres_model(lib, lights=(LOW_SUN,)):
    spec = rr.many_spheres_spec()
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    rc.add_spec(lib, b, spec, rc.palette(len(spec), seed=6))
    rc.far_body(lib, b)
    rc.add_camera(lib, b, b"above", 0, rc.VIEW_SPHERES)
    for L in lights:
        add_light(lib, b, 0, L)
    return rc.compile_model(lib, b)


def hfield_model(lib, lights=(HF_SUN,)):
    import ctypes as C
    b = lib.mjh_builder_create()
    el = (C.c_double * rr.HF_ELEV.size)(*rr.HF_ELEV.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", rr.HF_NROW, rr.HF_NCOL, D(*rr.HF_SIZE), el)
    g = lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*rr.HF_POS), D(*rr.HF_QUAT), None, -1, -1, -1)
    assert h >= 0 and g >= 0 and lib.mjh_builder_set_geom_rgba(b, g, D(0.3, 0.7, 0.2, 1.0)) == 0
    rc.far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    rc.add_camera(lib, b, b"cam", 0, rc.VIEW_HFIELD)
    for L in lights:
        add_light(lib, b, 0, L)
    return rc.compile_model(lib, b)


def meshes_model(lib, lights=(MESH_SUN,)):
    """render_check.meshes_model's scene (a floor, a tilted torus, a jaw, a flat quad, seen from above), with lights"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=[0, 0, 0])
    assert lib.mjh_builder_add_geom(b, b"floor", 0, rr.PLANE, D(0.0, 0.0, 0.05), D(0, 0, 0), None, None, -1, -1, -1, -1) >= 0
    for k, (mesh, pos, quat) in enumerate([("torus", (0.0, 0.0, rc.MESH_HEIGHT), rc.TORUS_QUAT), ("jaw", (1.1, 0.0, rc.MESH_HEIGHT), None), ("flat_quad", (-1.1, 0.0, rc.MESH_HEIGHT), None)]):
        asset = rt.add_mesh(lib, b, *rt.MESHES[mesh]())
        bd = lib.mjh_builder_add_body(b, b"mb%d" % k, 0, D(*pos), None if quat is None else D(*quat), 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, bd, asset, None, None, None, -1, -1, -1, -1) >= 0
    view = rc.VIEW_MESHES
    assert lib.mjh_builder_add_camera(b, b"cam", 0, D(*view[0]), D(*rc.mat2quat(rc.look_at(view[0], view[1]))), float(view[2])) >= 0
    for L in lights:
        add_light(lib, b, 0, L)
    m = rc.compile_model(lib, b)
    return m, tuple(m.name2id(2, "mg%d" % k) for k in range(3))


def model_lights(m, active=None):
    """the model's lights in the world at qpos0 (bodies that hang on the world)"""
    return lr.world_lights(m, m.array("body_pos").reshape(-1, 3), m.array("body_quat").reshape(-1, 4), active)


def device_lights(e, m, env, active=None):
    """... from the device's own body poses in env `env`"""
    xp, xq = e.get_body_state(env, 1)
    return lr.world_lights(m, xp[0], xq[0], active)


# ------------------------------------------------------------------ the comparison
def colour_tolerance(diffuse, lights):
    K = diffuse + sum(float(np.max(L["diffuse"])) for L in lights)
    return 2 + math.ceil(255 * K * math.sqrt(3.0) * rc.TOL_N)


def kept_pixels(name, scene, rays, lights, bias=BIAS, shadows=True, cutoff=0.0):
    """(centre reference, term [nl, npix, 3], cast-shadow mask, kept [npix], excluded share): asserts the cap.  cutoff: the view's far
    plane (depth along the optical axis: the ray parameter) — a hit beyond it is a miss, one within 1e-3 of it is left out"""
    centre, keep, _ = rc.kept_pixels(name, scene, rays)
    if cutoff > 0:
        d, g, n, f = centre
        far = d > cutoff
        keep = keep & (np.abs(d - cutoff) > 1e-3)
        centre = (np.where(far, -1.0, d), np.where(far, -1, g), np.where(far[:, None], 0.0, n), f)
    term, cast = lr.terms(lights, rays, scene, centre, bias, shadows)
    stable = np.ones(len(keep), bool)
    for sh in rf.shifted(rays):
        t, _ = lr.terms(lights, sh, scene, None, bias, shadows)
        stable &= (np.abs(t - term).max(axis=(0, 2)) <= TERM_TOL) if len(lights) else True
    for f in (0.5, 2.0):
        t, _ = lr.terms(lights, rays, scene, centre, bias * f, shadows)
        stable &= (np.abs(t - term).max(axis=(0, 2)) <= TERM_TOL) if len(lights) else True
    if cutoff > 0:
        stable |= far      # (beyond the far plane the pixel is a miss whatever the lights do)
    keep = keep & stable
    share = 1.0 - keep.mean()
    print(f"{name}: light-stable share {stable.mean():.4f}, excluded share with lights {share:.4f}, cast-shadow pixels per light (kept) {[int((c & keep).sum()) for c in cast]}")
    assert share <= CAP, (name, share)
    return centre, term, cast, keep, share


def check_light(name, gid, rgba, scene, rays, colours, lights, bias=BIAS, shadows=True, ambient=0.3, diffuse=0.7, background=(0.0, 0.0, 0.0, 0.0), tol=None, cutoff=0.0):
    """ONE env's colour image of lighting mode 1 against the reference.  Returns (worst colour difference, excluded share, kept
    cast-shadow pixels per light)"""
    npix = len(rays[0])
    gid = np.asarray(gid).reshape(npix); c = np.asarray(rgba).reshape(npix, 4).astype(int)
    centre, term, cast, keep, share = kept_pixels(name, scene, rays, lights, bias, shadows, cutoff)
    _, ref_g, ref_n, _ = centre
    assert (gid[keep] == ref_g[keep]).all(), name
    hit, khit = gid >= 0, keep & (ref_g >= 0)
    assert (c[~hit] == rf.level(np.asarray(background, np.float32))).all(), f"{name}: a miss has the background colour exactly"
    assert (c[hit, 3] == 255).all(), name
    ref_c = lr.colour(colours, ref_g, ref_n, np.asarray(rays[1], float), term, ambient, diffuse, background).astype(int)
    diff = np.abs(c[khit] - ref_c[khit])
    worst = int(diff.max(initial=0))
    allowed = colour_tolerance(diffuse, lights) if tol is None else tol
    print(f"{name}: kept hits {int(khit.sum())}, max colour difference {worst} (allowed {allowed})")
    assert worst <= allowed, (name, worst)
    return worst, share, [int((s & keep).sum()) for s in cast]
