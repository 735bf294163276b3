"""The texture kernel's own code (csrc/dev_texture.h, __host__ __device__) on the CPU: tests/texture_host/texture_host.hip built as a
shared object — the depth and shade kernels' code as tests/render_host runs it, then a lane of mjh_texture_kernel and the shade
kernel's textured colour per ray — against the fp64 reference tests/texture_ref.py, by the comparison of tests/texture_check.py.  No GPU.

The scenes, views and image sizes are the GPU tests' own (tests/test_gpu_texture.py) and the 64 x 48 views, at qpos0, with poses, sizes
and rays rounded to float32.  On kept hits the texel bytes equal the reference's exactly; the worst colour difference is asserted to be
within texture_check.C_HOST_TEX and printed (`pytest tests/test_texture_host.py -s`).  The lit route is not rebuilt on the host: the
light kernel takes the texel through the same render_texel_base.

The same source with its own main runs once under AddressSanitizer / UBSan (a stand-alone program: nothing is loaded into Python
under a sanitizer)."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import ray_ref as rr
import render_check as rc
import texture_check as tc
from test_render_host import Host as RenderHost, f32_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "texture_host", "texture_host.hip")
TEXEL_FLAG = 0xff000000


def pack(textures):
    """(words [ntexdata] uint32 as the engine packs them, adr per texture)"""
    words, adr = [], []
    n = 0
    for t in textures:
        t = np.asarray(t).reshape(-1, 3).astype(np.uint32)
        adr.append(n); n += len(t)
        words.append(t[:, 0] | (t[:, 1] << 8) | (t[:, 2] << 16) | np.uint32(TEXEL_FLAG))
    return np.ascontiguousarray(np.concatenate(words), np.uint32), adr


class Host(RenderHost):
    """texture_host_image through render_host_image's own argument marshalling"""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.texture_host_image.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8 + \
            [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        self.lib.texture_host_image.restype = C.c_int
        self._tex = None

        def image(*a):      # render_host_image's arguments: ..., background, outputs
            head, outs = a[:27], a[27:]
            rec, words, self._word = self._tex
            return self.lib.texture_host_image(*head, rec.ctypes.data, words.ctypes.data, len(words), *outs, self._word.ctypes.data)
        self.lib.render_host_image = image

    def textured(self, m, scene, rays, textures, records, **kw):
        """(depth, gid, normal, rgba, texel words) of the textured image"""
        words, adr = pack(textures)
        rec = np.zeros((m.ngeom, 8), np.float32)
        for g, R in enumerate(records):
            t = R["tex"]
            rec[g] = [t, adr[t] if t >= 0 else 0, textures[t].shape[1] if t >= 0 else 1, textures[t].shape[0] if t >= 0 else 1, R["repeat"][0], R["repeat"][1], float(R["uniform"]), 0]
        self._tex = (rec, words, np.zeros(len(rays[0]), np.uint32))
        out = self.render(m, scene, rays, **kw)
        return out + (self._tex[2],)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Host(hostbuild.shared(SRC, tmp_path_factory.mktemp("texture_host")))


@pytest.fixture(scope="module")
def models(lib):
    return dict(white=(tc.prim_model(lib), tc.prim_textures()), prim=(tc.prim_model(lib, coloured=True), tc.prim_textures()),
                spheres=(tc.spheres_model(lib), tc.spheres_textures()), hfield=(tc.hfield_model(lib), tc.hfield_textures()))


# (model, camera, width, height): the images tests/test_gpu_texture.py renders, and the 64 x 48 views
IMAGES = [("prim", "front", 30, 20), ("prim", "front", 8, 8), ("prim", "front", 9, 8), ("prim", "front", 1, 1), ("prim", "front", 64, 48),
          ("prim", "side", 30, 20), ("prim", "side", 8, 8), ("prim", "side", 9, 8), ("prim", "side", 1, 1), ("prim", "side", 64, 48),
          ("spheres", "above", 16, 16), ("hfield", "cam", 30, 20)]


@pytest.mark.parametrize("name,cam,width,height", IMAGES, ids=[f"{a}-{b}-{c}x{d}" for a, b, c, d in IMAGES])
def test_c_host_over_the_gpu_scenes(host, models, name, cam, width, height):
    m, textures = models[name]
    records = tc.model_records(m)
    scene = f32_scene(rc.model_scene(m))
    rays = rr.f32(*rc.model_camera_rays(m, m.name2id(5, cam), width, height))
    depth, gid, nrm, rgba, word = host.textured(m, scene, rays, textures, records)
    worst, ntex, share, added = tc.check_colour(f"host {name} {cam} {width}x{height}", gid, rgba, scene, rays, rc.model_colours(m), textures, records, tol=tc.C_HOST_TEX)
    print(f"C_HOST_TEX candidate {worst}, kept textured hits {ntex}, excluded share {share:.4f}, the texel rule adds {added:.4f}")
    # the texel image itself: on kept hits the reference's bytes and the flag, no flag on an untextured geom or a miss
    centre, _, t0, has, keep, _, _ = tc.kept_pixels(f"host {name} {cam} {width}x{height}", scene, rays, textures, records)
    khit = keep & (centre[1] >= 0)
    got = np.stack([word & 0xff, (word >> 8) & 0xff, (word >> 16) & 0xff], axis=1).astype(int)
    assert ((word[khit & has] & TEXEL_FLAG) == TEXEL_FLAG).all() and (got[khit & has] == t0[khit & has]).all(), "the host build's texels are the reference's"
    assert (word[khit & ~has] == 0).all() and (word[gid < 0] == 0).all()
    if (width, height) == (30, 20):
        assert ntex >= 100, "the comparison sees textured pixels"


@pytest.mark.parametrize("cam,width,height", [("front", 30, 20), ("side", 30, 20), ("side", 9, 8), ("side", 1, 1)])
def test_flat_image_is_the_texel(host, models, cam, width, height):
    """ambient 1, diffuse 0, white geoms: the colour image holds the texels' bytes"""
    m, textures = models["white"]
    records = tc.model_records(m)
    scene = f32_scene(rc.model_scene(m))
    rays = rr.f32(*rc.model_camera_rays(m, m.name2id(5, cam), width, height))
    depth, gid, nrm, rgba, word = host.textured(m, scene, rays, textures, records, ambient=1.0, diffuse=0.0)
    ntex, _, _ = tc.check_texels(f"host flat {cam} {width}x{height}", gid, rgba, scene, rays, textures, records)
    if (width, height) == (30, 20):
        kinds = {int(g) for g in np.unique(gid[(word & TEXEL_FLAG) != 0])}
        assert ntex >= 100 and kinds >= {0, 5}, "the floor and the box show their textures"


def test_sanitized_program(tmp_path):
    out = hostbuild.sanitized_run(SRC, "TEXTURE_HOST_MAIN", tmp_path)
    print(out)
    pixels, textured = int(out.split()[0]), int(out.split()[2])
    assert pixels > 200000 and textured > 1000
