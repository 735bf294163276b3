"""The device's own analytic pair routines (csrc/dev_collide.h, __host__ __device__) on the CPU: tests/collide_host/collide_host.hip
built as a shared object and checked with the independent fp64 geometry of tests/pairgeom.py, and built as a stand-alone program with
AddressSanitizer / UBSan on its host part.  No GPU.

The families of tests/test_pairgeom.py, 20 000 cases each, at the device test's tolerance (1e-5 on `dist` and surface membership,
tests/test_gpu_pairs.py); the reference geoms are the float32 poses handed to the routine, cast to float64.  A plane family draws 20
plane poses; a round family takes 2 500 generated pairs through 8 rigid motions each (the true distance stays, every float32
operand changes).  The x86 build does not contract to FMA as the device build does: this is a rehearsal of the arithmetic and of
the control flow; the device figures are those of tests/test_gpu_pairs.py.

What this found in the parent's routines (same cases, same reference):
  * c_capsule_capsule: 104 of 20 000 fail, all with axes closer than 1e-3 rad (det is pure noise below about 3e-4 rad), `dist` up to 4.5e-4 m above the true distance and
    contact points up to 1e-2 m off the capsules: in fp32 `det = ma mc - mb mb` of such axes is rounding noise (+-6e-8) or exactly 0,
    x1, x2 = noise / noise land anywhere inside their ranges, where no clamp repairs them, and the parallel branch is off by
    angle x length.  One alternating round after the clamps left 90 failures (worst 7.3e-5).  Since the edge minima of the
    parameter box are compared with the pair: 0, `dist` at most 7.2e-7 above the true distance.
  * c_plane_cylinder: 599 of 19 786 robust cases fail, all within 1e-1 rad of standing, passing only from 1e-3: the rim direction
    keeps an axial remainder of rounding size, which lifts the rim point off the cap.  Since it is taken out again: 0.
Every family now passes from the first rung of the ladder, 1e-6 (`passes from` in the run's output); the non-robust share is at
most 1.6 % (plane_mesh)."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import pairgeom as pg
from pairmodels import CAP, mesh_cloud, needed_tol, summarize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "collide_host", "collide_host.hip")
TOL = 1e-5
NCASE = 20000
LADDER = [1e-6 * 10 ** (k / 2) for k in range(12)]
MAXCON = 4


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(hostbuild.shared(SRC, tmp_path_factory.mktemp("collide_host")))
    fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int)
    lib.collide_host_batch.argtypes = [C.c_int, C.c_int, fp, fp, fp, C.c_int, fp, fp, fp, C.c_float, fp, ip]
    lib.collide_host_batch.restype = None
    lib.collide_host_set_mesh.argtypes = [fp, C.c_int]
    mesh = np.ascontiguousarray(mesh_cloud(), dtype=np.float32)
    lib.collide_host_set_mesh(mesh.ctypes.data_as(fp), len(mesh))

    def run(t1, t2, A, margin=0.0):
        n = len(A[0])
        out = np.zeros((n, MAXCON, 7), dtype=np.float32); cnt = np.zeros(n, dtype=np.int32)
        P = [a.ctypes.data_as(fp) for a in A]
        lib.collide_host_batch(n, t1, P[0], P[1], P[2], t2, P[3], P[4], P[5], margin, out.ctypes.data_as(fp), cnt.ctypes.data_as(ip))
        return cnt, out.astype(np.float64)
    run.mesh = mesh
    return run


def host_cases(family, n, seed=20261018):
    """(geom pairs, tags) of a family in world frames of their own"""
    rng = np.random.default_rng(seed)
    mesh = mesh_cloud().astype(np.float32).astype(np.float64)
    out = []
    if family.startswith("plane_"):
        for k in range(20):
            plane = (np.array([1.0, 0, 0, 0]) if k == 0 else pg.rand_quat(rng), rng.uniform(-0.3, 0.3, 3))
            out += [(c["g1"], c["g2"], c["tag"]) for c in pg.cases(family, n // 20, seed + k, plane=plane, mesh=mesh)]
        return out
    for c in pg.cases(family, n // 8, seed):
        for k in range(8):
            Q, T = (np.eye(3), np.zeros(3)) if k == 0 else (pg.quat_mat(pg.rand_quat(rng)), rng.uniform(-0.4, 0.4, 3))
            out.append(tuple((g[0], Q @ g[1] + T, Q @ g[2], g[3]) for g in (c["g1"], c["g2"])) + (c["tag"],))
    return out


def run_family(host, family, n, margin=0.0):
    cs = host_cases(family, n)
    t1, t2 = cs[0][0][0], cs[0][1][0]
    f32 = lambda x: np.ascontiguousarray(x, dtype=np.float32)
    size = lambda g: np.zeros(3) if g[0] in (pg.PLANE, pg.MESH) else g[3][:3]
    A = [f32([c[0][1] for c in cs]), f32([c[0][2].reshape(-1) for c in cs]), f32([size(c[0]) for c in cs]),
         f32([c[1][1] for c in cs]), f32([c[1][2].reshape(-1) for c in cs]), f32([size(c[1]) for c in cs])]
    cnt, out = host(t1, t2, A, margin)
    rows = []; excess = 0.0
    for i, c in enumerate(cs):
        gs = tuple((c[k][0], A[3*k][i].astype(float), A[3*k+1][i].astype(float).reshape(3, 3),
                    host.mesh.astype(float) if c[k][0] == pg.MESH else A[3*k+2][i].astype(float)) for k in range(2))
        k = cnt[i]
        dist, pos, nrm = out[i, :k, 0], out[i, :k, 1:4], out[i, :k, 4:7]
        D = pg.true_distance(gs[0], gs[1])
        rob = pg.robust(gs[0], gs[1], margin, D=D)
        need = needed_tol(gs[0], gs[1], dist, pos, nrm, LADDER, margin, D) if rob else 0.0
        bad = pg.check_contacts(gs[0], gs[1], margin, dist, pos, nrm, tol=TOL, D=D) if need > TOL else []
        if rob and k == 1 and t1 != pg.PLANE:
            excess = max(excess, dist[0] - D)
        rows.append((rob, k > 0, bad, need, c[2]))
    if t1 != pg.PLANE:
        print(f"PAIRGEOM host fp32 {family}: worst dist above the true distance {excess:.3e}")
    return rows


@pytest.mark.parametrize("family", pg.FAMILIES)
def test_host_build_passes_the_independent_geometry_check(host, family):
    rows = run_family(host, family, NCASE)
    nrob, ntouch, fails, worst = summarize(f"host fp32 {family}", rows, TOL)
    assert len(rows) >= NCASE and nrob >= (1 - CAP) * len(rows) and ntouch >= 0.5 * len(rows)
    assert not fails, (len(fails), fails[:5])


def test_a_margin_brings_in_separated_pairs(host):
    """the same check with a margin of 2 mm: contacts with positive dist up to the margin, none beyond"""
    for family in ("sphere_capsule", "plane_box", "capsule_capsule"):
        rows = run_family(host, family, 2000, margin=0.002)
        nrob, ntouch, fails, worst = summarize(f"host fp32 {family} margin 2e-3", rows, TOL)
        assert nrob >= (1 - CAP) * len(rows) and not fails, (family, nrob, fails[:5])


def test_sanitized_stand_alone_run_is_clean(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): 2e5 calls over the ten routines, aligned
    orientations and coincident centres among them, into an exactly-sized staging array"""
    hostbuild.sanitized_run(SRC, "COLLIDE_HOST_MAIN", tmp_path)
