"""What tests/test_texture_host.py (the texture kernel's code on the CPU) and tests/test_gpu_texture.py (mjh_render with texturing
mode 1 on the device) share: the textured models, and the comparison of ONE env's colour image with tests/texture_ref.py.

The comparison.  A pixel is KEPT where render_check.kept_pixels (lit images: light_check.kept_pixels) keeps it AND the reference's texel
bytes at the four 1e-4-shifted rays of render_ref.shifted equal the centre ray's (a pixel on a texel's edge is left out).  The share left
out is asserted to be at most ray_check.CAP = 0.02.  On every kept hit of the flat image (ambient 1, diffuse 0, white geoms) R, G, B
equal the reference texel's bytes exactly; on every kept hit of a shaded or lit image each channel is within the allowance of that
route WITHOUT textures (render_check.colour_tolerance / light_check.colour_tolerance): the texel is exact on a kept pixel and the extra
product geom_rgba * (t / 255) is formed in float32 by the reference as the definition states it.  A miss is the background exactly,
alpha is 255.

The inputs keep the reference alone within the cap: the floor carries the 512 x 512 checker (four constant regions) at texrepeat 1 1,
uniform, with its frame shifted off the 1 m lattice (FLOOR_POS: the side view's 1 x 1 ray meets the unshifted floor at x = -2, on a
texel edge); the small geoms carry 8 x 8 textures of distinct bytes.  A non-uniform texture at texrepeat 1 1 puts the faces x = +-a_x
and y = +-a_y of a box (and the walls of a height field) exactly on the seam u = 0 / 1, where the rounding of the hit point picks the
column: the non-uniform records use REPEAT = (0.9, 0.8), which puts those faces in the middle of a texel.

C_HOST_TEX is the worst colour difference over the kept pixels of every image of tests/test_texture_host.py (the host build of
csrc/dev_texture.h and the shade kernel's colour code against this reference).  Measured there: 0 levels in every image, and on every kept
hit the host build's texel bytes are the reference's; C_HOST_TEX = 1 leaves the host build one rounding step.  On one MI355X
(tests/test_gpu_texture.py): the flat images hold the reference's texel bytes on every kept hit (28 compared images), the shaded and lit
images differ by 0 levels in all 20 compared images (allowed 2 and 3).

Excluded shares measured on the CPU (the same test; share / of which the texel rule adds): primitives front 30 x 20 0 / 0, 8 x 8 0 / 0,
9 x 8 0 / 0, 1 x 1 0 / 0, 64 x 48 0.0003 / 0; side 30 x 20 0.0033 / 0, 8 x 8 0.0156 (one pixel of 64) / 0, 9 x 8 0 / 0, 1 x 1 0 / 0,
64 x 48 0.0020 / 0.0007; with the lights of light_check the same figures; 70 spheres over the infinite textured floor 16 x 16 0 / 0; the
textured height field 30 x 20 0.0033 / 0.0017.  On the device's poses (four envs, spread free bodies): at most 0.0156, the texel rule
adding at most 0.0017."""
import numpy as np

import light_check as lc
import light_ref as lr
import ray_ref as rr
import render_check as rc
import render_ref as rf
import texture_ref as tr
from helpers import D, set_opt
from ray_check import CAP

NENV = rc.NENV
C_HOST_TEX = 1        # levels: worst host-build colour difference (one rounding step is left to the host build; measured 0)
FLOOR_POS = (0.13, 0.07, 0.0)
REPEAT = (0.9, 0.8)
CHECKER = dict(kind=tr.CHECKER, width=512, height=512, rgb1=(0.1, 0.2, 0.3), rgb2=(0.2, 0.3, 0.4))      # the reference's "grid" texture


def distinct(seed, width=8, height=8):
    """a texture of width x height texels, no two alike, no byte 0 (a black texel could hide a missing product)"""
    k = np.arange(width * height)
    t = np.stack([(3 * k + 17 + seed) % 200 + 40, (197 - 2 * k - seed) % 200 + 30, (7 * k + 5 * seed + 11) % 190 + 60], axis=1)
    assert len({tuple(x) for x in t}) == len(t)
    return t.reshape(height, width, 3).astype(np.uint8)


def add_texture(lib, b, name, tex):
    import ctypes as C
    t = np.ascontiguousarray(tex, np.uint8)
    tid = lib.mjh_builder_add_texture(b, name, t.shape[1], t.shape[0], t.ctypes.data_as(C.POINTER(C.c_ubyte)))
    assert tid >= 0, lib.mjh_last_error()
    return tid


def add_builtin(lib, b, name, kind, width, height, rgb1=None, rgb2=None, mark=tr.NONE, markrgb=None):
    tid = lib.mjh_builder_add_texture_builtin(b, name, kind, mark, width, height, None if rgb1 is None else D(*rgb1), None if rgb2 is None else D(*rgb2),
                                              None if markrgb is None else D(*markrgb))
    assert tid >= 0, lib.mjh_last_error()
    return tid


def textured_spec():
    spec = rr.primitives_spec()
    spec[0] = dict(spec[0], pos=FLOOR_POS)
    return spec


# spec index -> (texture index, repeat, uniform): the floor, the static sphere, cylinder and box, the free box
PRIM_TEXTURED = {0: (0, (1.0, 1.0), 1), 1: (1, (1.0, 1.0), 1), 4: (2, REPEAT, 0), 5: (3, REPEAT, 0), 10: (3, REPEAT, 0)}
FREE_BOX = 10


def prim_textures():
    return [tr.builtin(**CHECKER), distinct(1), distinct(2), distinct(3)]


def prim_model(lib, coloured=False, textured=True, lights=(), gravity=(0, 0, 0)):
    """render_check.prim_model's scene (the floor's frame shifted to FLOOR_POS) with white or palette colours; textured: the floor carries
    the checker, one sphere, one cylinder and two boxes 8 x 8 textures of distinct bytes; lights on the world body"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=list(gravity))
    spec = textured_spec()
    rc.add_spec(lib, b, spec, rc.palette(len(spec)) if coloured else np.ones((len(spec), 4)))
    rc.add_camera(lib, b, b"front", 0, rc.VIEW_FRONT)
    rc.add_camera(lib, b, b"side", 0, rc.VIEW_SIDE)
    if textured:
        ids = [add_builtin(lib, b, b"grid", CHECKER["kind"], CHECKER["width"], CHECKER["height"], CHECKER["rgb1"], CHECKER["rgb2"])]
        ids += [add_texture(lib, b, b"t%d" % k, distinct(k)) for k in (1, 2, 3)]
        # (rc.add_spec adds the geoms in spec order: the builder's geom id is the spec index)
        for g, (t, rep, uni) in PRIM_TEXTURED.items():
            assert lib.mjh_builder_set_geom_texture(b, g, ids[t], D(*rep), uni) == 0, lib.mjh_last_error()
    for L in lights:
        lc.add_light(lib, b, 0, L)
    return rc.compile_model(lib, b)


SECOND_PASS = (69, 70)


def spheres_model(lib, textured=True):
    """render_check.spheres_model (more than 64 geoms: two staging passes of the depth launch) over a textured floor"""
    spec = rr.many_spheres_spec()
    spec[0] = dict(spec[0], pos=FLOOR_POS)
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    rc.add_spec(lib, b, spec, rc.palette(len(spec), seed=6))
    rc.far_body(lib, b)
    rc.add_camera(lib, b, b"above", 0, rc.VIEW_SPHERES)
    if textured:
        t = add_builtin(lib, b, b"grid", CHECKER["kind"], CHECKER["width"], CHECKER["height"], CHECKER["rgb1"], CHECKER["rgb2"])
        s = add_texture(lib, b, b"t4", distinct(4))
        # the floor is an infinite plane (size 0 0): not uniform, its half extents count as 1
        assert lib.mjh_builder_set_geom_texture(b, 0, t, D(1.0, 1.0), 0) == 0
        for g in SECOND_PASS:      # spheres of the second staging pass that the 16 x 16 view sees
            assert lib.mjh_builder_set_geom_texture(b, g, s, D(1.0, 1.0), 1) == 0
    return rc.compile_model(lib, b)


def spheres_textures():
    return [tr.builtin(**CHECKER), distinct(4)]


def hfield_model(lib):
    """render_check.hfield_model with an 8 x 8 texture on the terrain (not uniform: the asset's half extents)"""
    import ctypes as C
    b = lib.mjh_builder_create()
    el = (C.c_double * rr.HF_ELEV.size)(*rr.HF_ELEV.ravel())
    h = lib.mjh_builder_add_hfield(b, b"terrain", rr.HF_NROW, rr.HF_NCOL, D(*rr.HF_SIZE), el)
    g = lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*rr.HF_POS), D(*rr.HF_QUAT), None, -1, -1, -1)
    assert h >= 0 and g >= 0 and lib.mjh_builder_set_geom_rgba(b, g, D(0.3, 0.7, 0.2, 1.0)) == 0
    rc.far_body(lib, b)
    set_opt(lib, b, gravity=[0, 0, 0])
    rc.add_camera(lib, b, b"cam", 0, rc.VIEW_HFIELD)
    t = add_texture(lib, b, b"t5", distinct(5))
    assert lib.mjh_builder_set_geom_texture(b, g, t, D(*REPEAT), 0) == 0, lib.mjh_last_error()
    return rc.compile_model(lib, b)


def hfield_textures():
    return [distinct(5)]


def model_records(m):
    """the geoms' texture records from the model's tables"""
    tid, rep, uni = m.array("geom_texid"), m.array("geom_texrepeat").reshape(-1, 2), m.array("geom_texuniform")
    assert len(tid) == m.ngeom
    return [dict(tex=int(tid[g]), repeat=(float(rep[g, 0]), float(rep[g, 1])), uniform=bool(uni[g])) for g in range(m.ngeom)]


def model_textures(m):
    """the model's textures as [H, W, 3] arrays (the tests compare them with the arrays they were made from)"""
    w, h, adr, rgb = m.array("tex_width"), m.array("tex_height"), m.array("tex_adr"), m.array("tex_rgb").reshape(-1, 3)
    return [rgb[adr[t]:adr[t] + w[t] * h[t]].reshape(h[t], w[t], 3) for t in range(m.ntex)]


# ------------------------------------------------------------------ the comparison
def texel_stable(scene, rays, centre, textures, records):
    """(texel bytes [npix, 3], textured [npix], stable [npix]) of the reference: stable where the four shifted rays give the centre's bytes"""
    d, g = centre[0], centre[1]
    t0, has = tr.texels(textures, records, scene, g, tr.hit_points(rays, d, g))
    stable = np.ones(len(g), bool)
    for sh in rf.shifted(rays):
        ds, gs, _, _ = rf.cast(sh[0], sh[1], scene)
        ts, hs = tr.texels(textures, records, scene, gs, tr.hit_points(sh, ds, gs))
        stable &= (ts == t0).all(axis=1) & (hs == has)
    return t0, has, stable


def kept_pixels(name, scene, rays, textures, records, lights=None, **kw):
    """(centre, term or None, texel bytes, textured, kept, excluded share, share the texel rule adds): asserts the cap"""
    if lights is None:
        centre, keep, _ = rc.kept_pixels(name, scene, rays)
        term = None
    else:
        centre, term, _, keep, _ = lc.kept_pixels(name, scene, rays, lights, **kw)
    t0, has, stable = texel_stable(scene, rays, centre, textures, records)
    added = float((keep & ~stable).mean())
    keep = keep & stable
    share = 1.0 - keep.mean()
    print(f"{name}: textured pixels {int(has.sum())}, excluded share with the texel rule {share:.4f} (the rule adds {added:.4f})")
    assert share <= CAP, (name, share)
    return centre, term, t0, has, keep, share, added


def check_texels(name, gid, rgba, scene, rays, textures, records, background=(0.0, 0.0, 0.0, 0.0)):
    """ONE env's flat image (ambient 1, diffuse 0, white geoms): on kept hits the texel's bytes exactly, 255 on an untextured geom.
    Returns (kept textured hits, excluded share, added share)"""
    npix = len(rays[0])
    gid = np.asarray(gid).reshape(npix); c = np.asarray(rgba).reshape(npix, 4).astype(int)
    centre, _, t0, has, keep, share, added = kept_pixels(name, scene, rays, textures, records)
    ref_g = centre[1]
    assert (gid[keep] == ref_g[keep]).all(), name
    hit, khit = gid >= 0, keep & (ref_g >= 0)
    assert (c[~hit] == rf.level(np.asarray(background, np.float32))).all(), f"{name}: a miss has the background colour exactly"
    assert (c[hit, 3] == 255).all(), name
    want = np.where(has[:, None], t0, 255)
    bad = int((c[khit, :3] != want[khit]).any(axis=1).sum())
    print(f"{name}: kept hits {int(khit.sum())}, textured {int((khit & has).sum())}, hits with other bytes than the reference texel {bad}")
    assert bad == 0, (name, bad)
    return int((khit & has).sum()), share, added


def check_colour(name, gid, rgba, scene, rays, colours, textures, records, lights=None, ambient=0.3, diffuse=0.7, background=(0.0, 0.0, 0.0, 0.0), tol=None, **kw):
    """ONE env's shaded (lights None) or lit colour image against the reference.  Returns (worst colour difference, kept textured hits,
    excluded share, added share)"""
    npix = len(rays[0])
    gid = np.asarray(gid).reshape(npix); c = np.asarray(rgba).reshape(npix, 4).astype(int)
    centre, term, t0, has, keep, share, added = kept_pixels(name, scene, rays, textures, records, lights, **kw)
    d, ref_g, ref_n, _ = centre
    assert (gid[keep] == ref_g[keep]).all(), name
    hit, khit = gid >= 0, keep & (ref_g >= 0)
    assert (c[~hit] == rf.level(np.asarray(background, np.float32))).all(), f"{name}: a miss has the background colour exactly"
    assert (c[hit, 3] == 255).all(), name
    # the references' colour functions take a colour per geom: here every pixel is its own "geom" with its albedo
    alb = tr.albedo(colours, textures, records, scene, ref_g, tr.hit_points(rays, d, ref_g))
    px = np.where(ref_g >= 0, np.arange(npix), -1)
    V = np.asarray(rays[1], float)
    if lights is None:
        ref_c = rf.colour(alb, px, ref_n, V, ambient, diffuse, background).astype(int)
        allowed = rc.colour_tolerance(diffuse) if tol is None else tol
    else:
        ref_c = lr.colour(alb, px, ref_n, V, term, ambient, diffuse, background).astype(int)
        allowed = lc.colour_tolerance(diffuse, lights) if tol is None else tol
    worst = int(np.abs(c[khit] - ref_c[khit]).max(initial=0))
    print(f"{name}: kept hits {int(khit.sum())}, textured {int((khit & has).sum())}, max colour difference {worst} (allowed {allowed})")
    assert worst <= allowed, (name, worst)
    return worst, int((khit & has).sum()), share, added
