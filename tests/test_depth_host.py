"""The depth kernel's ray generation and tile cull (csrc/dev_depth.h, __host__ __device__) on the CPU: tests/depth_host/depth_host.hip
built as a shared object.  No GPU.

Pixel directions: each component within 2e-7 relative of the fp64 formula d = (a t (2 (j + 1/2) / W - 1), t (1 - 2 (i + 1/2) / H), -1)
(the fp32 code rounds `scale` once and the product once: 2^-23 = 1.2e-7 at the most).
Cull: on 20 000 random (tile, sphere) cases per image size, whenever a pixel-centre ray of the tile meets the sphere in fp64 the
predicate keeps the sphere — zero exceptions; the share of spheres culled among those no ray hits is printed, not asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "depth_host", "depth_host.hip")
SIZES = [(1, 1), (8, 8), (30, 20), (64, 48)]      # (width, height)
FOVY = [20.0, 60.0, 120.0]


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(hostbuild.shared(SRC, tmp_path_factory.mktemp("depth_host")))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.depth_host_dirs.argtypes = [C.c_int, C.c_int, C.c_float, fp]
    lib.depth_host_dirs.restype = None
    lib.depth_host_cull.argtypes = [C.c_int, C.c_int, C.c_float, C.c_int, ip, ip, fp, fp, ip]
    lib.depth_host_cull.restype = None
    return lib


def scale_of(fovy, height):
    """what the engine hands the kernel: tan(fovy / 2) / height, rounded to fp32 once"""
    return np.float32(np.tan(np.radians(fovy) / 2) / height)


def dirs64(width, height, fovy):
    t, a = np.tan(np.radians(fovy) / 2), width / height
    i, j = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    return np.stack([a * t * (2 * (j + 0.5) / width - 1), t * (1 - 2 * (i + 0.5) / height), -np.ones((height, width))], axis=-1)


@pytest.mark.parametrize("fovy", FOVY)
@pytest.mark.parametrize("width,height", SIZES)
def test_pixel_directions_match_the_fp64_formula(host, width, height, fovy):
    out = np.zeros((height, width, 3), dtype=np.float32)
    host.depth_host_dirs(width, height, scale_of(fovy, height), out.ctypes.data_as(C.POINTER(C.c_float)))
    ref = dirs64(width, height, fovy)
    assert np.array_equal(out[..., 2], -np.ones((height, width), dtype=np.float32))
    err = np.abs(out.astype(float) - ref)
    rel = err / np.maximum(np.abs(ref), 1e-300)
    # a centre pixel of an odd image has a component that is exactly 0 in both
    rel[ref == 0] = err[ref == 0]
    print(f"{width}x{height} fovy {fovy}: worst relative component error {rel.max():.3g}")
    assert rel.max() <= 2e-7


@pytest.mark.parametrize("width,height", SIZES)
def test_cull_never_drops_a_sphere_a_pixel_ray_hits(host, width, height):
    rng = np.random.default_rng(1000 * width + height)
    n = 20000
    tx, ty = (width + 7) // 8, (height + 7) // 8
    kept_total = hit_total = culled_nohit = nohit = 0
    for fovy in FOVY:
        D = dirs64(width, height, fovy)
        trow, tcol = rng.integers(0, ty, n).astype(np.int32), rng.integers(0, tx, n).astype(np.int32)
        # sphere centres all around the camera (behind it too), radii from pixel-sized to larger than the distance (camera inside)
        u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
        # half of them aimed near the tile so that grazing cases are common
        near = rng.random(n) < 0.5
        ti = np.minimum(trow * 8 + rng.integers(0, 8, n), height - 1); tj = np.minimum(tcol * 8 + rng.integers(0, 8, n), width - 1)
        aim = D[ti, tj] / np.linalg.norm(D[ti, tj], axis=1, keepdims=True)
        u = np.where(near[:, None], aim + 0.15 * rng.normal(size=(n, 3)), u); u /= np.linalg.norm(u, axis=1, keepdims=True)
        dist = 10 ** rng.uniform(-1, 1, n)
        c = (u * dist[:, None]).astype(np.float32)
        r = (dist * 10 ** rng.uniform(-2.5, 0.1, n)).astype(np.float32)
        keep = np.zeros(n, dtype=np.int32)
        ip, fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
        host.depth_host_cull(width, height, scale_of(fovy, height), n, trow.ctypes.data_as(ip), tcol.ctypes.data_as(ip), c.ctypes.data_as(fp),
                             r.ctypes.data_as(fp), keep.ctypes.data_as(ip))
        # fp64: does any pixel-centre ray of the tile (origin at the apex) meet the sphere?
        c64, r64 = c.astype(float), r.astype(float)
        hit = np.zeros(n, bool)
        for di in range(8):
            for dj in range(8):
                i, j = trow * 8 + di, tcol * 8 + dj
                ok = (i < height) & (j < width)
                d = D[np.minimum(i, height - 1), np.minimum(j, width - 1)]
                d = d / np.linalg.norm(d, axis=1, keepdims=True)
                h = np.einsum("ij,ij->i", c64, d)
                q2 = np.einsum("ij,ij->i", c64, c64) - h * h
                inside = np.einsum("ij,ij->i", c64, c64) <= r64 * r64
                hit |= ok & (inside | ((h >= 0) & (q2 <= r64 * r64)))
        missed = hit & (keep == 0)
        assert not missed.any(), f"fovy {fovy}: {missed.sum()} spheres a pixel ray hits were culled, first case {np.flatnonzero(missed)[0]}"
        kept_total += int(keep.sum()); hit_total += int(hit.sum())
        nohit += int((~hit).sum()); culled_nohit += int(((~hit) & (keep == 0)).sum())
    assert hit_total > 1000      # (the cases do exercise the contract)
    print(f"{width}x{height}: {hit_total} of {3 * n} spheres hit by a pixel ray, all kept; culled {culled_nohit} of the {nohit} no ray hits "
          f"({100.0 * culled_nohit / max(nohit, 1):.1f} %)")
