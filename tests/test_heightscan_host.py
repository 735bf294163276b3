"""The height-scan kernel's grid code (csrc/dev_heightscan.h: the host checks and the __host__ __device__ functions) on the CPU:
tests/heightscan_host/heightscan_host.hip built as a shared object.  No GPU.

Frames: every entry of the grid frame within 4e-7 of the fp64 rule applied to the same fp32 rotation (a normalisation is a square
root, a division and a product: three roundings of at most 2^-24 = 6e-8 on values of at most 1, with room); a site whose x axis is
exactly vertical gives the world frame in YAW alignment.
Cells: within 4 * 2^-24 E of the fp64 formula, E = |offset| + (size - 1) / 2 * spacing the grid's extent: the offset and half the
spacing are rounded to fp32 once each (the second scaled by an integer of at most size - 1) and the fused multiply-add rounds once.
Cull: on 20 000 random (pose, alignment, tile, sphere) cases per grid, whenever a live ray of the tile, as a half-line from its start
in fp64, meets the sphere, hscan_tile_keep keeps it — zero exceptions; the share culled among the spheres no ray meets is printed, not
asserted.
Argument checks: what mjh_heightscan refuses, decided by the function the engine calls.
Sanitizers: the same source as a stand-alone program under AddressSanitizer / UBSan (tests/hostbuild.py)."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import heightscan_ref as hr
import hostbuild
import ray_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "heightscan_host", "heightscan_host.hip")
fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(hostbuild.shared(SRC, tmp_path_factory.mktemp("heightscan_host")))
    lib.hscan_host_check.argtypes = [C.c_int] * 9 + [dp, dp, C.c_double, C.c_int, C.c_int, C.c_int]; lib.hscan_host_check.restype = C.c_int
    lib.hscan_host_frames.argtypes = [C.c_int, ip, fp, fp]; lib.hscan_host_frames.restype = None
    lib.hscan_host_cells.argtypes = [C.c_int, C.c_int] + [C.c_float] * 4 + [fp, fp]; lib.hscan_host_cells.restype = None
    lib.hscan_host_cull.argtypes = [C.c_int, C.c_int] + [C.c_float] * 5 + [C.c_int, fp, fp, ip, ip, fp, fp, ip]; lib.hscan_host_cull.restype = None
    return lib


def frames(host, align, S32):
    n = len(align)
    a = np.ascontiguousarray(align, dtype=np.int32); S32 = np.ascontiguousarray(S32, dtype=np.float32)
    G = np.zeros((n, 9), dtype=np.float32)
    host.hscan_host_frames(n, a.ctypes.data_as(ip), S32.ctypes.data_as(fp), G.ctypes.data_as(fp))
    return G.reshape(n, 3, 3)


def grid32(grid):
    """the grid as the engine hands it to the kernel: offset and half the spacing rounded to fp32 once, and `above`"""
    _, _, spacing, offset, above = grid
    return np.float32(offset[0]), np.float32(offset[1]), np.float32(0.5 * spacing[0]), np.float32(0.5 * spacing[1]), np.float32(above)


def random_rotations(rng, n):
    return np.array([rr.quat2mat(rr.random_quat(rng)) for _ in range(n)]).astype(np.float32)


def test_grid_frames_match_the_fp64_rule(host):
    rng = np.random.default_rng(7)
    n = 3000
    S32 = random_rotations(rng, n)
    # some x axes close to vertical, on either side of the fallback's threshold (but not on it)
    for k in range(0, 200):
        tilt = 10 ** rng.uniform(-5, -1.5)
        ax = np.array([tilt * np.cos(k), tilt * np.sin(k), (-1) ** k * np.sqrt(1 - tilt * tilt)])
        ay = np.cross([0.3, 0.5, 0.1], ax); ay /= np.linalg.norm(ay)
        S32[k] = np.stack([ax, ay, np.cross(ax, ay)], axis=1).ravel().astype(np.float32)
    l2 = S32[:, 0].astype(float) ** 2 + S32[:, 3].astype(float) ** 2
    assert (np.abs(l2 - hr.DEGENERATE) > 1e-9).all(), "no case sits on the threshold, where fp32 and fp64 may decide differently"
    assert (l2 < hr.DEGENERATE).sum() > 20 and ((l2 > hr.DEGENERATE) & (l2 < 1e-3)).sum() > 20
    worst = 0.0
    for name in hr.ALIGNS:
        G = frames(host, np.full(n, hr.ALIGN_ID[name]), S32)
        ref = np.array([hr.grid_frame(S.astype(float).reshape(3, 3), name) for S in S32])
        err = np.abs(G.astype(float) - ref).max()
        worst = max(worst, err)
        print(f"{name}: worst absolute entry error {err:.3g}")
        if name != "base":
            assert (G[:, :, 2] == np.array([0.0, 0.0, 1.0], dtype=np.float32)).all(), "gz is exactly the world's z: the rays go along (0, 0, -1)"
        if name == "base":
            assert np.array_equal(G.reshape(n, 9), S32)
    assert worst <= 4e-7


def test_a_vertical_x_axis_falls_back_to_the_world_x(host):
    for sign in (1.0, -1.0):
        S = np.array([[0, 0, sign], [0, 1, 0], [-sign, 0, 0]], dtype=np.float32)      # x axis = (0, 0, -sign): exactly vertical
        G = frames(host, [hr.ALIGN_ID["yaw"]], S.reshape(1, 9))[0]
        assert np.array_equal(G, np.eye(3, dtype=np.float32))
        assert np.array_equal(hr.grid_frame(S.astype(float), "yaw"), np.eye(3))
        assert np.array_equal(frames(host, [hr.ALIGN_ID["base"]], S.reshape(1, 9))[0], S)


@pytest.mark.parametrize("name", list(hr.GRIDS))
def test_cell_coordinates(host, name):
    for grid in (hr.GRIDS[name], hr.GRIDS[name][:3] + ((-37.123, 912.7),) + hr.GRIDS[name][4:]):
        width, height, spacing, offset, above = grid
        ox, oy, hx, hy, _ = grid32(grid)
        x = np.zeros(width, dtype=np.float32); y = np.zeros(height, dtype=np.float32)
        host.hscan_host_cells(width, height, ox, oy, hx, hy, x.ctypes.data_as(fp), y.ctypes.data_as(fp))
        rx, ry = hr.cells(grid)
        ex = abs(offset[0]) + (width - 1) / 2 * spacing[0]; ey = abs(offset[1]) + (height - 1) / 2 * spacing[1]
        errx, erry = np.abs(x - rx).max(), np.abs(y - ry).max()
        print(f"{name} offset {offset}: x error {errx:.3g} (extent {ex:.3g}), y error {erry:.3g} (extent {ey:.3g})")
        assert errx <= 4 * 2.0 ** -24 * ex and erry <= 4 * 2.0 ** -24 * ey
        assert (np.diff(x) > 0).all() and (np.diff(y) > 0).all() if min(width, height) > 1 else True, "column 0 is the lowest x, row 0 the lowest y"


@pytest.mark.parametrize("name", list(hr.GRIDS))
def test_cull_never_drops_a_sphere_a_ray_hits(host, name):
    grid = hr.GRIDS[name]
    width, height, spacing, offset, above = grid
    th, tw = hr.tile_shape(height)
    tx, ty = (width + tw - 1) // tw, (height + th - 1) // th
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = 20000
    ox, oy, hx, hy, ab = grid32(grid)
    # a sensor pose per case: up to 30 m from the world's origin (the slack must carry the origins' rounding there), any orientation
    o32 = (rng.uniform(-1, 1, (n, 3)) * 10 ** rng.uniform(-1, 1.5, (n, 1))).astype(np.float32)
    S32 = random_rotations(rng, n)
    align = rng.integers(0, 3, n).astype(np.int32)
    G32 = frames(host, align, S32)
    G = np.array([hr.grid_frame(S32[k].astype(float).reshape(3, 3), hr.ALIGNS[align[k]]) for k in range(n)])      # fp64, columns gx gy gz
    u = -G[:, :, 2] / np.linalg.norm(G[:, :, 2], axis=1, keepdims=True)
    x, y = hr.cells(grid)
    trow, tcol = rng.integers(0, ty, n).astype(np.int32), rng.integers(0, tx, n).astype(np.int32)

    def start(i, j):      # fp64 start points of cell (i[k], j[k]) of case k
        return o32.astype(float) + G[:, :, 0] * x[j][:, None] + G[:, :, 1] * y[i][:, None] + G[:, :, 2] * above

    # sphere centres: half of them near a ray of the tile (before, at and beyond its start) so that grazing cases are common, the
    # others anywhere around the sensor; radii from 0.3 % of the distance to beyond it (the start inside)
    ti = np.minimum(trow * th + rng.integers(0, th, n), height - 1); tj = np.minimum(tcol * tw + rng.integers(0, tw, n), width - 1)
    near = rng.random(n) < 0.5
    t = rng.uniform(-0.5, 5.0, n)
    c_near = start(ti, tj) + u * t[:, None] + rng.normal(size=(n, 3)) * 10 ** rng.uniform(-2.5, -0.5, (n, 1))
    c_far = o32.astype(float) + rng.uniform(-4, 4, (n, 3))
    c = np.where(near[:, None], c_near, c_far).astype(np.float32)
    dist = np.linalg.norm(c.astype(float) - start(ti, tj), axis=1)
    r = (np.maximum(dist, 0.02) * 10 ** rng.uniform(-2.5, 0.1, n)).astype(np.float32)
    keep = np.zeros(n, dtype=np.int32)
    host.hscan_host_cull(width, height, ox, oy, hx, hy, ab, n, o32.ctypes.data_as(fp), np.ascontiguousarray(G32).ctypes.data_as(fp),
                         trow.ctypes.data_as(ip), tcol.ctypes.data_as(ip), c.ctypes.data_as(fp), r.ctypes.data_as(fp), keep.ctypes.data_as(ip))
    # fp64: does any live ray of the tile, a half-line from its start, meet the sphere?
    c64, r64 = c.astype(float), r.astype(float)
    hit = np.zeros(n, bool)
    for di in range(th):
        for dj in range(tw):
            i, j = trow * th + di, tcol * tw + dj
            ok = (i < height) & (j < width)
            d = c64 - start(np.minimum(i, height - 1), np.minimum(j, width - 1))
            dd = np.einsum("ij,ij->i", d, d); h = np.einsum("ij,ij->i", d, u)
            hit |= ok & ((dd <= r64 * r64) | ((h >= 0) & (dd - h * h <= r64 * r64)))
    missed = hit & (keep == 0)
    assert not missed.any(), f"{missed.sum()} spheres a ray hits were culled, first case {np.flatnonzero(missed)[0]}"
    assert hit.sum() > 1000      # (the cases do exercise the contract)
    nohit = int((~hit).sum()); culled = int(((~hit) & (keep == 0)).sum())
    print(f"{name}: tiles {th} x {tw}; {int(hit.sum())} spheres hit by a ray, all kept; culled {culled} of the {nohit} no ray hits "
          f"({100.0 * culled / max(nohit, 1):.1f} %)")


def test_argument_checks(host):
    def bad(nsite=1, nbody=3, nenv=4, env0=0, n=4, site=0, align=0, width=16, height=16, spacing=(0.1, 0.1), offset=(0.0, 0.0), above=1.0,
            bodyexclude=-1, exclude_tree=0, null=False):
        sp = (C.c_double * 2)(*spacing); off = (C.c_double * 2)(*offset)
        return host.hscan_host_check(nsite, nbody, nenv, env0, n, site, align, width, height, sp, off, above, bodyexclude, exclude_tree, int(null))

    assert bad() == 0
    assert bad(site=-1) == 0 and bad(bodyexclude=2, exclude_tree=1) == 0 and bad(bodyexclude=0, exclude_tree=1) == 0
    assert bad(align=1) == 0 and bad(align=2) == 0 and bad(above=-3.0) == 0 and bad(offset=(-5.0, 1e6)) == 0
    assert bad(width=1 << 14, height=1 << 14, n=3) == 0, "3 * 2^28 cells are below the limit"
    for kw in (dict(site=1), dict(site=-2), dict(bodyexclude=3), dict(bodyexclude=-2), dict(exclude_tree=1), dict(exclude_tree=1, bodyexclude=-1),
               dict(align=3), dict(align=-1), dict(width=0), dict(height=0), dict(width=-4), dict(height=-1),
               dict(width=1 << 14, height=1 << 14, n=4), dict(width=1 << 15, height=1 << 15, n=1),
               dict(spacing=(0.0, 0.1)), dict(spacing=(0.1, -0.1)), dict(spacing=(np.nan, 0.1)), dict(spacing=(0.1, np.inf)), dict(spacing=(1e-60, 0.1)),
               dict(offset=(np.nan, 0.0)), dict(offset=(0.0, -np.inf)), dict(above=np.nan), dict(above=np.inf), dict(above=1e39),
               dict(offset=(1e39, 0.0)), dict(spacing=(1e37, 0.1), width=100), dict(spacing=(0.1, 3e38), height=4),
               dict(env0=2, n=3), dict(env0=-1, n=2), dict(env0=4, n=1), dict(n=0), dict(n=-1), dict(env0=2 ** 31 - 1, n=2), dict(null=True)):
        assert bad(**kw) == 1, kw


def test_grid_code_is_clean_under_the_sanitizers(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): frames, cells and cylinders of six grids in
    three alignments out of heap buffers of exactly the documented sizes, every ray inside its own tile's cylinder, and the checks"""
    out = hostbuild.sanitized_run(SRC, "HEIGHTSCAN_HOST_MAIN", tmp_path)
    print(out.strip())
    assert "rays in" in out
