"""The scan kernel's pattern code (csrc/dev_scan.h: host functions and __host__ __device__ ones) on the CPU: tests/scan_host/scan_host.hip
built as a shared object.  No GPU.

Beam directions: each component within 2e-7 absolute of the fp64 formula d = (cos el cos az, cos el sin az, sin el) — the two table
entries carry one fp32 rounding each and the product a third, each at most 2^-24 = 6e-8 on values of at most 1.
Cone: on 20 000 random (tile, sphere) cases per pattern, whenever a live beam of the tile meets the sphere in fp64 the kernel's decision
(scan_tile_cone, then depth_cone_keep where the tile has a cone) keeps the sphere — zero exceptions; the share culled among the
spheres no beam meets is printed, not asserted.
Pattern checks: what mjh_scan refuses, decided by the function the engine calls.
Sanitizers: the same source as a stand-alone program under AddressSanitizer / UBSan (tests/hostbuild.py), tables of exactly the
documented sizes."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest

import hostbuild
import scan_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "scan_host", "scan_host.hip")
fp, ip, dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(hostbuild.shared(SRC, tmp_path_factory.mktemp("scan_host")))
    lib.scan_host_tile_shape.argtypes = [C.c_int]; lib.scan_host_tile_shape.restype = C.c_int
    lib.scan_host_check.argtypes = [C.c_int, C.c_int, C.c_longlong, C.c_double, C.c_double, dp, C.c_double, C.c_double]; lib.scan_host_check.restype = C.c_int
    lib.scan_host_tables.argtypes = [C.c_int, C.c_int, C.c_double, C.c_double, dp, C.c_double, C.c_double, fp]; lib.scan_host_tables.restype = None
    lib.scan_host_dirs.argtypes = [C.c_int, C.c_int, fp, fp]; lib.scan_host_dirs.restype = None
    lib.scan_host_cull.argtypes = [C.c_int, C.c_int, fp, C.c_float, C.c_int, ip, ip, fp, fp, ip, ip]; lib.scan_host_cull.restype = None
    return lib


def _el_args(el):
    """(table pointer or None, elevation0, elevation_step, the array that backs the pointer)"""
    if isinstance(el, tuple):
        return None, el[0], el[1], None
    t = np.ascontiguousarray(el, dtype=np.float64)
    return t.ctypes.data_as(dp), 0.0, 0.0, t


def tables(host, pattern):
    width, height, az0, step, el = pattern
    ptr, e0, es, keep = _el_args(el)
    assert host.scan_host_check(width, height, 1, az0, step, ptr, e0, es) == 0
    tab = np.zeros(2 * (width + height), dtype=np.float32)
    host.scan_host_tables(width, height, az0, step, ptr, e0, es, tab.ctypes.data_as(fp))
    return tab


def test_tile_shape_follows_the_pattern_height(host):
    for height, th in [(1, 1), (2, 2), (3, 4), (4, 4), (5, 8), (8, 8), (9, 8), (16, 8), (1000, 8)]:
        assert 64 >> host.scan_host_tile_shape(height) == th == sr.tile_shape(height)[0]


@pytest.mark.parametrize("name", list(sr.PATTERNS))
def test_beam_directions_match_the_fp64_formula(host, name):
    pattern = sr.PATTERNS[name]
    width, height = pattern[:2]
    tab = tables(host, pattern)
    az, el = sr.angles(pattern)
    ref_tab = np.concatenate([np.cos(az), np.sin(az), np.cos(el), np.sin(el)])
    assert np.array_equal(tab, ref_tab.astype(np.float32)) or np.abs(tab - ref_tab).max() <= 2.0 ** -24, "the tables are the fp64 values rounded once"
    out = np.zeros((height, width, 3), dtype=np.float32)
    host.scan_host_dirs(width, height, tab.ctypes.data_as(fp), out.ctypes.data_as(fp))
    ref = sr.beams64(pattern)
    err = np.abs(out.astype(float) - ref).max()
    norm = np.abs(np.linalg.norm(out.astype(float), axis=-1) - 1).max()
    print(f"{name}: worst absolute component error {err:.3g}, worst | |d| - 1 | {norm:.3g}")
    assert err <= 2e-7
    assert norm <= 4e-7, "a unit vector up to rounding"


@pytest.mark.parametrize("name", list(sr.CONE_PATTERNS))
def test_cull_never_drops_a_sphere_a_beam_hits(host, name):
    pattern = sr.CONE_PATTERNS[name]
    width, height, az0, step, _ = pattern
    th, tw = sr.tile_shape(height)
    tx, ty = (width + tw - 1) // tw, (height + th - 1) // th
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    n = 20000
    tab = tables(host, pattern)
    Dn = sr.beams64(pattern)      # unit vectors
    trow, tcol = rng.integers(0, ty, n).astype(np.int32), rng.integers(0, tx, n).astype(np.int32)
    # sphere centres all around the sensor (above and below the poles too), half of them aimed near a beam of the tile so that grazing
    # cases are common; radii from 0.3 % of the distance to beyond it (the sensor inside)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    near = rng.random(n) < 0.5
    ti = np.minimum(trow * th + rng.integers(0, th, n), height - 1); tj = np.minimum(tcol * tw + rng.integers(0, tw, n), width - 1)
    u = np.where(near[:, None], Dn[ti, tj] + 0.15 * rng.normal(size=(n, 3)), u); u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = 10 ** rng.uniform(-1, 1, n)
    c = (u * dist[:, None]).astype(np.float32)
    r = (dist * 10 ** rng.uniform(-2.5, 0.1, n)).astype(np.float32)
    keep = np.zeros(n, dtype=np.int32); cone = np.zeros(n, dtype=np.int32)
    host.scan_host_cull(width, height, tab.ctypes.data_as(fp), np.float32(abs(step)), n, trow.ctypes.data_as(ip), tcol.ctypes.data_as(ip),
                        c.ctypes.data_as(fp), r.ctypes.data_as(fp), keep.ctypes.data_as(ip), cone.ctypes.data_as(ip))
    # fp64: does any live beam of the tile (origin at the apex) meet the sphere?
    c64, r64 = c.astype(float), r.astype(float)
    cc = np.einsum("ij,ij->i", c64, c64)
    hit = np.zeros(n, bool)
    for di in range(th):
        for dj in range(tw):
            i, j = trow * th + di, tcol * tw + dj
            ok = (i < height) & (j < width)
            d = Dn[np.minimum(i, height - 1), np.minimum(j, width - 1)]
            h = np.einsum("ij,ij->i", c64, d)
            hit |= ok & ((cc <= r64 * r64) | ((h >= 0) & (cc - h * h <= r64 * r64)))
    missed = hit & (keep == 0)
    assert not missed.any(), f"{missed.sum()} spheres a beam hits were culled, first case {np.flatnonzero(missed)[0]}"
    assert hit.sum() > 1000      # (the cases do exercise the contract)
    nohit = int((~hit).sum()); culled = int(((~hit) & (keep == 0)).sum())
    print(f"{name}: tiles {th} x {tw}, {int(cone.sum())} of {n} cases in a tile with a cone; {int(hit.sum())} spheres hit by a beam, all kept; "
          f"culled {culled} of the {nohit} no beam hits ({100.0 * culled / max(nohit, 1):.1f} %)")
    span = (np.minimum(tw, width - tcol * tw) - 1) * abs(step)
    wide = span > np.pi
    assert not cone[wide].any() and keep[wide].all(), "a tile that spans more than pi in azimuth has no cone: everything is kept"
    if name == "3 columns 120 degrees":
        assert wide.all()
    if name in ("planar 1x1081", "full turn 16x360", "9x70"):      # (a tile that reaches from pole to pole has a cone of nearly 90 degrees)
        assert cone.all() and culled > 0.5 * nohit, "these patterns' tiles all have a cone, and it does cull"


def test_pattern_checks(host):
    def bad(width=4, height=3, n=2, az0=0.0, step=0.1, el=(0.0, 0.1)):
        ptr, e0, es, keep = _el_args(el)
        return host.scan_host_check(width, height, n, az0, step, ptr, e0, es)

    assert bad() == 0
    assert bad(el=np.array([np.pi / 2, -np.pi / 2, 0.0])) == 0 and bad(el=(-np.pi / 2, np.pi / 2)) == 0, "the poles themselves are rows"
    assert bad(step=0.0) == 0 and bad(step=-0.1) == 0
    for kw in (dict(width=0), dict(height=0), dict(width=-1), dict(height=-5), dict(width=1 << 15, height=1 << 14, n=2, el=(0.1, 0.0)), dict(width=1 << 16, height=1 << 14, n=1, el=(0.1, 0.0)),
               dict(az0=np.nan), dict(az0=np.inf), dict(step=np.nan), dict(step=-np.inf), dict(az0=1e308, step=1e308),
               dict(el=(np.nan, 0.1)), dict(el=(0.0, np.inf)), dict(el=(0.0, 1.0)), dict(el=(-1.6, 0.1)), dict(el=(1.0, -1.5)),
               dict(el=np.array([0.0, np.nan, 0.1])), dict(el=np.array([0.0, 1.58, 0.1])), dict(el=np.array([-1.58, 0.0, 0.1])), dict(el=np.array([0.0, 0.1, np.inf]))):
        assert bad(**kw) == 1, kw
    assert bad(width=1 << 15, height=1 << 14, n=1, el=(0.1, 0.0)) == 0, "2^29 beams are below the limit"
    # cos el is never negative in the tables, at a pole neither
    tab = tables(host, (2, 3, 0.0, 0.1, (-np.pi / 2, np.pi / 2)))
    assert (tab[4:7] >= 0).all() and tab[4] < 1e-7 and tab[5] == 1.0


def test_pattern_code_is_clean_under_the_sanitizers(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): tables, directions and cones of eight patterns
    out of heap buffers of exactly the documented sizes, and every live beam inside its own tile's cone"""
    out = hostbuild.sanitized_run(SRC, "SCAN_HOST_MAIN", tmp_path)
    print(out.strip())
    assert "beams in" in out
