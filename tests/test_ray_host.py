"""The ray kernel's own intersection code (csrc/dev_ray.h, __host__ __device__) on the CPU: tests/ray_host/ray_host.hip built as a
shared object and compared with the fp64 reference (ray_ref.geom_ray, which brute-forces every triangle of a height field and shares
nothing with the kernel's cell walk), and built as a stand-alone program with AddressSanitizer / UBSan on its host part.  No GPU.

On the rays the reference finds robust (ray_ref.robust): same hit / miss and |dist - ref| <= 5e-5 max(1, ref), the tolerance of
tests/test_gpu_ray.py.  The x86 build does not contract to FMA as the device build does: this is a rehearsal of the arithmetic and
of the control flow; the device figures are those of tests/test_gpu_ray.py.

Before the cell walk took its cell coordinates from one expression with a tolerance that grows with the grid (an absolute 1e-6
before), the height-field families failed here, wrong / robust rays: A nodes 21 / 266, A row planes 45 / 598, B nodes 42 / 266,
B column planes 91 / 598 (C and every other family 0) — every such ray through the terrain onto the base.  Since: 0 in every family,
worst scaled error 3.1e-6."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import ray_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_host", "ray_host.hip")
TOL = 5e-5
PRIMS = [(rr.PLANE, (3.0, 2.0, 0.05))] + rr.PRIMITIVES
NAMES = {rr.PLANE: "plane", rr.SPHERE: "sphere", rr.CAPSULE: "capsule", rr.ELLIPSOID: "ellipsoid", rr.CYLINDER: "cylinder", rr.BOX: "box"}


def _hipcc():
    return shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    hipcc = _hipcc()
    assert hipcc, "hipcc is what builds this project"
    so = tmp_path_factory.mktemp("ray_host") / "libray_host.so"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O2", "-shared", "-fPIC", SRC, "-o", str(so)])
    lib = C.CDLL(str(so))
    fp = C.POINTER(C.c_float)
    lib.ray_host_cast.argtypes = [C.c_int, fp, C.c_int, C.c_int, fp, fp, C.c_int, fp, fp, fp]
    lib.ray_host_cast.restype = None

    def cast(t, size, P, V, hf=None):
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        P32, V32, s = a(P), a(V), a(size)
        assert np.array_equal(P32.astype(float), P) and np.array_equal(V32.astype(float), V), "the rays are float32 numbers already"
        out = np.full(len(P32), 7.0, dtype=np.float32)
        hs, el = (a(hf[2]), a(hf[3])) if hf is not None else (a(np.zeros(4)), a(np.zeros(1)))
        lib.ray_host_cast(t, s.ctypes.data_as(fp), hf[0] if hf else 0, hf[1] if hf else 0, hs.ctypes.data_as(fp), el.ctypes.data_as(fp), len(P32),
                          P32.ctypes.data_as(fp), V32.ctypes.data_as(fp), out.ctypes.data_as(fp))
        return out.astype(float)
    return cast


def _compare(name, got, t, size, rays, hf=None):
    """(wrong, robust, worst scaled error) of the host fp32 distances against the reference"""
    scene = rr.terrain_scene(hf) if hf is not None else dict(pos=np.zeros((1, 3)), mat=np.eye(3).reshape(1, 9), size=np.array([size], float),
                                                             type=np.array([t]), visible=np.ones(1, bool), hfield={})
    ref = rr.geom_ray(t, rays[0], rays[1], size, hf)
    rob = rr.robust(rays, scene)
    hit = ref >= 0
    err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
    wrong = rob & (((got >= 0) != hit) | (hit & (err > TOL)))
    worst = float(err[rob & hit & (got >= 0)].max()) if (rob & hit & (got >= 0)).any() else 0.0
    print(f"{name}: {len(rob)} rays, robust {int(rob.sum())}, hits {int((rob & hit).sum())}, wrong {int(wrong.sum())}, max scaled error {worst:.3e}")
    return int(wrong.sum()), int(rob.sum()), worst


@pytest.mark.parametrize("t,size", PRIMS, ids=[NAMES[t] for t, _ in PRIMS])
def test_primitives_against_the_reference(host, t, size):
    bad = []
    for dist in (3.0, 30.0):
        for k, fam in enumerate(rr.FRAME_FAMILIES):
            rays = rr.frame_rays(t, size, fam, dist, 4000, seed=1000 * t + 10 * k + int(dist))
            got = host(t, size, *rays)
            wrong, nrob, _ = _compare(f"{NAMES[t]} {fam} {dist:g} m", got, t, size, rays)
            assert nrob >= 0.9 * len(got), (fam, dist)
            if wrong:
                bad.append((fam, dist, wrong))
    assert not bad, bad


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_hfield_families_against_the_reference(host, name):
    hf = rr.terrain(name)
    bad = []
    for fam, rays in rr.hfield_families(name, nrand=2000):
        got = host(rr.HFIELD, (0, 0, 0), *rays, hf=hf)
        wrong, nrob, _ = _compare(f"terrain {name} {fam}", got, rr.HFIELD, (0, 0, 0), rays, hf)
        assert nrob >= 0.9 * len(got), fam
        if wrong:
            bad.append((fam, wrong, nrob))
    assert not bad, bad


def test_interior_nodes_are_hit_on_the_top(host):
    """straight down at a node the distance is the origin's height minus the node's elevation"""
    for name in ("A", "B", "C"):
        hf = rr.terrain(name)
        P, V, rc = rr.hfield_node_rays(hf)
        got = host(rr.HFIELD, (0, 0, 0), P, V, hf=hf)
        want = (P[:, 2] - hf[3][rc[:, 0], rc[:, 1]] * hf[2][2]) / -V[:, 2]
        assert np.abs(got - want).max() <= TOL * max(1.0, want.max()), name


def test_sanitized_stand_alone_run_is_clean(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): 2e5 rays per terrain over an exactly-sized
    elevation array, border lines and corner nodes included, and the primitive families"""
    hipcc = _hipcc()
    assert hipcc
    probe = tmp_path / "probe.hip"
    probe.write_text("int main() { return 0; }\n")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]
    if subprocess.run([hipcc, "--offload-arch=gfx950", *san, str(probe), "-o", str(tmp_path / "probe")], capture_output=True).returncode != 0:
        pytest.skip("AddressSanitizer / UBSan runtime not available to hipcc")
    exe = tmp_path / "ray_host_san"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-DRAY_HOST_MAIN", *san, SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1"))
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[:4000]
    assert r.returncode == 0, (r.returncode, r.stdout, r.stderr[:2000])
    assert r.stderr.strip() == "", r.stderr[:2000]
    assert " 0 failures" in r.stdout
