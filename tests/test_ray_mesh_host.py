"""The ray kernel's own half-space clipping (csrc/dev_ray.h: ray_convex, __host__ __device__) on the CPU: tests/ray_host/
ray_mesh_host.hip built as a shared object and compared with the fp64 reference (ray_mesh_ref: scipy's hull triangles, which share
nothing with the clipping nor with the builder's hull), and built as a stand-alone program with AddressSanitizer / UBSan on its host
part.  No GPU.

The planes are the compiled model's (mesh_plane), rounded to float32 as the engine uploads them; the reference sees the fp64 kept
vertices.  On the rays the reference finds robust (ray_mesh_ref.robust): same hit / miss and |dist - ref| <= 5e-5 max(1, ref), the
project's ray tolerance (tests/test_gpu_ray.py).  The share of non-robust rays is a property of the ray sets alone; it is asserted here
(<= 10 % per family) so that the device tests can reuse the sets.  The x86 build does not contract to FMA as the device build does: this
is a rehearsal of the arithmetic and of the control flow.

Measured: 0 wrong rays in every family, worst scaled error 6.0e-7 (ellipsoid points, through edge, 3 m); largest non-robust share 0.068
(PR2's largest mesh, in face plane: the one ray in 25 that lies in the facet's plane exactly, plus a few that graze an edge)."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import ray_mesh_ref as rm
import ray_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_host", "ray_mesh_host.hip")
TOL = 5e-5
NRAY = 400


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    lib = C.CDLL(hostbuild.shared(SRC, tmp_path_factory.mktemp("ray_mesh_host")))
    fp = C.POINTER(C.c_float)
    lib.ray_mesh_host_cast.argtypes = [fp, C.c_int, C.c_int, fp, fp, fp]
    lib.ray_mesh_host_cast.restype = None

    def cast(planes, P, V):
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        pl, P32, V32 = a(planes), a(P), a(V)
        assert np.array_equal(P32.astype(float), P) and np.array_equal(V32.astype(float), V), "the rays are float32 numbers already"
        out = np.full(len(P32), 7.0, dtype=np.float32)
        lib.ray_mesh_host_cast(pl.ctypes.data_as(fp), len(pl), len(P32), P32.ctypes.data_as(fp), V32.ctypes.data_as(fp), out.ctypes.data_as(fp))
        return out.astype(float)
    return cast


@pytest.fixture(scope="module")
def meshes(lib):
    """name -> (kept vertices fp64, planes of the compiled model): the shared meshes (a) - (c) and PR2's largest mesh (most planes)"""
    out = {}
    for name, pts in (("box", rm.box_points()), ("tetrahedron", rm.tetra_points()), ("ellipsoid points", rm.ellipsoid_points())):
        m = rm.mesh_only_model(lib, pts)
        out[name] = (rm.model_mesh_verts(m)[0], rm.model_mesh_planes(m)[0])
    m = rm.load_robot(lib, "pr2")
    k = int(np.argmax(m.array("mesh_planenum")))
    out["pr2 largest"] = (rm.model_mesh_verts(m)[k], rm.model_mesh_planes(m)[k])
    assert len(out["pr2 largest"][1]) >= 100
    return out


@pytest.mark.parametrize("name", ["box", "tetrahedron", "ellipsoid points", "pr2 largest"])
def test_ray_convex_against_the_reference(host, meshes, name):
    vert, planes = meshes[name]
    scene = rm.single_mesh_scene(vert)
    bad, shares = [], []
    for dist in (3.0, 30.0):
        for k, fam in enumerate(rm.MESH_FAMILIES):
            rays = rm.mesh_rays(vert, fam, dist, NRAY, seed=1000 + 10 * k + int(dist))
            got = host(planes, *rays)
            ref, _ = rm.cast(rays[0], rays[1], scene)
            rob = rm.robust(rays, scene)
            hit = ref >= 0
            err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
            wrong = rob & (((got >= 0) != hit) | (hit & (err > TOL)))
            ok = rob & hit & (got >= 0)
            worst = float(err[ok].max()) if ok.any() else 0.0
            share = 1.0 - rob.mean()
            print(f"{name} {fam} {dist:g} m: {len(rob)} rays, non-robust share {share:.3f}, hits {int((rob & hit).sum())}, wrong {int(wrong.sum())}, max scaled error {worst:.3e}")
            shares.append((fam, dist, share))
            assert (got[~hit & rob] == -1.0).all(), (fam, dist)
            assert (rob & hit).sum() >= NRAY // 4, (fam, dist, "the family hits the mesh")
            if wrong.any():
                bad.append((fam, dist, int(wrong.sum())))
    assert all(s <= 0.10 for _, _, s in shares), shares
    assert not bad, bad


def test_an_origin_inside_hits_the_far_face_and_parallel_rays(host, meshes):
    _, planes = meshes["box"]
    P = rr.f32(np.array([[0.05, 0.02, -0.03], [0.0, 0.0, 1.0], [0.0, 0.0, 1.0], [0.5, 0.0, 1.0], [1.0, 0.15, 0.0], [1.0, 0.1500001, 0.0], [1.0, 0.0, 0.0]]))
    V = rr.f32(np.array([[0, 0, 2.0], [0, 0, -0.5], [0, 0, 1.0], [0, 0, -1.0], [-1.0, 0, 0], [-1.0, 0, 0], [-1.0, 0, 0]]))
    got = host(planes, P, V)
    assert got[0] == pytest.approx(0.13 / 2.0, abs=1e-6)      # from inside: the far face
    assert got[1] == pytest.approx(1.8, abs=1e-6)
    assert got[2] == -1.0 and got[3] == -1.0                  # pointing away; passing beside the box (den == 0, num < 0 on a side face)
    assert got[4] == pytest.approx(0.8, abs=1e-6)             # in the plane of the face y = 0.15 (den == 0, num == 0): the face belongs to the box
    assert got[5] == -1.0                                     # one float32 step outside that plane
    assert got[6] == pytest.approx(0.8, abs=1e-6)


def test_sanitized_stand_alone_run_is_clean(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): plane sets of every length 1 .. 13 and of 55,
    150 and 666 planes in exactly-sized heap arrays, rays from 3 m and 30 m, from inside, with zero components, along the axes and
    in the plane of a face"""
    hostbuild.sanitized_run(SRC, "RAY_MESH_HOST_MAIN", tmp_path)
