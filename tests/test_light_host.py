"""The light kernel's own code (csrc/dev_light.h, __host__ __device__) on the CPU: tests/light_host/light_host.hip built as a shared
object — the depth and shade kernels' code as tests/render_host runs it, then mjh_light_kernel's tile loop — against the fp64 reference
tests/light_ref.py, by the comparison of tests/light_check.py.  No GPU.

The scenes, lights and image sizes are the GPU tests' own (tests/test_gpu_light.py), at qpos0, with poses, sizes, rays and lights rounded
to float32.  Every case asserts the cap on the excluded share and the colour bound, prints the measured worst difference, and checks
that cull on and off give the same bytes.  `pytest tests/test_light_host.py -s` prints every case; the values are recorded beside
C_HOST in light_check.py and in DESIGN.md section 4d."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import light_check as lc
import light_ref as lr
import ray_ref as rr
import render_check as rc
from test_render_host import Host as RenderHost, f32_scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "light_host", "light_host.hip")


class Host(RenderHost):
    """light_host_image through render_host_image's own argument marshalling"""

    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.light_host_image.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8 + \
            [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 4
        self.lib.light_host_image.restype = C.c_int
        self._lights = None

        def image(*a):      # render_host_image's arguments: ..., nray, P, V, range, ambient, diffuse, background, outputs
            head, (nray, P, V, range_, ambient, diffuse, bg), outs = a[:20], a[20:27], a[27:]
            width, height, lights, shadows, cull, bias = self._lights
            assert nray == width * height and not range_
            return self.lib.light_host_image(*head, width, height, P, V, ambient, diffuse, bg, len(lights), lights.ctypes.data, shadows, cull, bias, *outs)
        self.lib.render_host_image = image

    def light(self, m, scene, rays, width, height, lights, surface=None, shadows=1, cull=1, bias=lc.BIAS, **kw):
        rec = np.zeros((max(len(lights), 1), 16), np.float32)
        for k, L in enumerate(lights):
            rec[k] = list(L["pos"]) + list(L["dir"]) + list(L["diffuse"]) + list(L["ambient"]) + [np.cos(np.radians(L["cutoff"])), L["exponent"], float(L["directional"]), float(L["castshadow"])]
        self._lights = (width, height, rec[:len(lights)].copy() if len(lights) else rec[:0], int(shadows), int(cull), float(bias))
        return self.render(m, scene, rays, surface, **kw)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Host(hostbuild.shared(SRC, tmp_path_factory.mktemp("light_host")))


@pytest.fixture(scope="module")
def models(lib):
    out = dict(prim=lc.prim_model(lib), low=lc.prim_model(lib, lights=(lc.LOW_SPOT,)), spheres=lc.spheres_model(lib), hfield=lc.hfield_model(lib))
    out["meshes"], out["mesh_geoms"] = lc.meshes_model(lib)
    return out


# (model, mesh surface, camera, width, height): the images tests/test_gpu_light.py renders, and the 64 x 48 views
IMAGES = [("prim", None, "front", 30, 20), ("prim", None, "front", 8, 8), ("prim", None, "front", 9, 8), ("prim", None, "front", 1, 1), ("prim", None, "front", 64, 48),
          ("prim", None, "side", 30, 20), ("prim", None, "side", 8, 8), ("prim", None, "side", 9, 8), ("prim", None, "side", 1, 1), ("prim", None, "side", 64, 48),
          ("low", None, "front", 30, 20), ("low", None, "side", 30, 20), ("spheres", None, "above", 16, 16), ("hfield", None, "cam", 30, 20),
          ("meshes", 0, "cam", 24, 16), ("meshes", 1, "cam", 24, 16)]


@pytest.mark.parametrize("name,surface,cam,width,height", IMAGES, ids=[f"{a}-{b}-{c}-{d}x{e}" for a, b, c, d, e in IMAGES])
def test_c_host_over_the_gpu_scenes(host, models, name, surface, cam, width, height):
    m = models[name]
    scene = f32_scene(rc.model_scene(m, surface))
    rays = rr.f32(*rc.model_camera_rays(m, m.name2id(5, cam), width, height))
    lights = lr.f32_lights(lc.model_lights(m))
    depth, gid, nrm, rgba = host.light(m, scene, rays, width, height, lights, surface)
    worst, share, shadowed = lc.check_light(f"host {name} surface {surface} {cam} {width}x{height}", gid, rgba, scene, rays, rc.model_colours(m), lights)
    print(f"C_HOST candidate {worst}, excluded share {share:.4f}, kept cast-shadow pixels per light {shadowed}")
    assert worst <= lc.C_HOST
    if (width, height) == (30, 20) and name == "prim":
        assert min(shadowed) >= 8, "both lights cast shadows the comparison sees"
    # cull off: the same bytes
    off = host.light(m, scene, rays, width, height, lights, surface, cull=0)
    assert off[3].tobytes() == rgba.tobytes(), "the cull costs no hit"
    # shadows off against the reference without shadow rays
    ns = host.light(m, scene, rays, width, height, lights, surface, shadows=0)
    lc.check_light(f"host {name} {cam} {width}x{height}, no shadows", ns[1], ns[3], scene, rays, rc.model_colours(m), lights, shadows=False)
    if max(shadowed) > 0:
        assert ns[3].tobytes() != rgba.tobytes()


def test_no_light_is_the_shade_kernels_image(host, models):
    """without lights the sum is 0.0f: the colour is the shade kernel's up to the rounding of |n . v^| from the stored normal"""
    m = models["prim"]
    scene = f32_scene(rc.model_scene(m))
    rays = rr.f32(*rc.model_camera_rays(m, 0, 30, 20))
    lit = host.light(m, scene, rays, 30, 20, [])
    lc.check_light("host prim front, no lights", lit[1], lit[3], scene, rays, rc.model_colours(m), [])


def test_torus_hole_passes_light_under_triangles_only(host, models):
    m, (g_torus, g_jaw, g_quad) = models["meshes"], models["mesh_geoms"]
    rays = rr.f32(*rc.model_camera_rays(m, 0, 24, 16))
    lights = lr.f32_lights(lc.model_lights(m))
    cast = {}
    for surface in (0, 1):
        scene = f32_scene(rc.model_scene(m, surface))
        centre, term, shadow, keep, _ = lc.kept_pixels(f"meshes surface {surface}", scene, rays, lights)
        cast[surface] = (centre[1], shadow[0], keep)
    floor_both = (cast[0][0] == 0) & (cast[1][0] == 0) & cast[0][2] & cast[1][2]
    lit_through = floor_both & cast[0][1] & ~cast[1][1]
    print(f"floor pixels shadowed by the hull and lit through the triangles: {int(lit_through.sum())}")
    assert lit_through.sum() >= 2, "the hull fills the torus's hole and the jaw's gap; the triangles let the light through"
