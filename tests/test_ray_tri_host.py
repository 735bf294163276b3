"""The ray kernels' own triangle walk (csrc/dev_ray.h: ray_tri, ray_trimesh, __host__ __device__) and the BVH builder (csrc/ray_bvh.h,
the file engine.hip includes) on the CPU: tests/ray_host/ray_tri_host.hip built as a shared object — the BVH's invariants, the walk
through the BVH against a loop of the same ray_tri over all triangles (bit for bit: pruning changes nothing), and both against the fp64
reference (ray_mesh_ref.tri_ray / cast / robust fed the model's mesh_tri) — and as a stand-alone program with AddressSanitizer / UBSan
on its host part.  No GPU.

On the rays the reference finds robust: same hit / miss and |dist - ref| <= 5e-5 max(1, ref), the project's ray tolerance
(tests/test_gpu_ray_mesh.py).  The share of non-robust rays is a property of the ray sets alone; it is asserted here (<= 10 % per set) so
that the device tests can reuse the sets.  The x86 build does not contract to FMA as the device build does: a rehearsal of the
arithmetic and of the control flow.

Measured: 0 wrong rays in every set, 0 rays where the BVH and the loop differ; worst scaled error 6.0e-6 (torus, through vertex; every
other set below 1e-6 but the torus's first general set, 4.5e-6); largest non-robust share 0.085 (sheet, in face plane: the one ray in 25
that lies in the facet's plane exactly, plus the open surface's rim); the rays at the torus's vertices and edge midpoints all hit, as do
those at the flat quad's edges (its in-plane family misses throughout, as the reference does)."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import ray_mesh_ref as rm
import ray_tri_ref as rt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_host", "ray_tri_host.hip")
TOL = 5e-5
NRAY = 400
NAMES = ["torus", "jaw", "sheet", "flat_quad", "box12", "five"]


class Host:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.fp, self.ip, self.dp = C.POINTER(C.c_float), C.POINTER(C.c_int), C.POINTER(C.c_double)
        self.lib.rth_build.argtypes = [self.dp, C.c_int]; self.lib.rth_build.restype = C.c_int
        self.lib.rth_get.argtypes = [self.fp, self.ip, self.ip, self.ip, self.fp, self.fp]; self.lib.rth_get.restype = None
        self.lib.rth_cast.argtypes = [C.c_int, self.fp, self.fp, self.fp, self.fp, self.fp]; self.lib.rth_cast.restype = None
        self.ntri = 0

    def build(self, tris):
        t = np.ascontiguousarray(tris, float).reshape(-1, 9)
        self.ntri = len(t)
        n = self.lib.rth_build(t.ctypes.data_as(self.dp), len(t))
        assert n > 0
        box = np.zeros((n, 6), np.float32); skip = np.zeros(n, np.int32); leaf = np.zeros(n, np.int32)
        order = np.zeros(len(t), np.int32); rec = np.zeros((len(t), 16), np.float32); rad = np.zeros(2, np.float32)
        self.lib.rth_get(box.ctypes.data_as(self.fp), skip.ctypes.data_as(self.ip), leaf.ctypes.data_as(self.ip), order.ctypes.data_as(self.ip),
                         rec.ctypes.data_as(self.fp), rad.ctypes.data_as(self.fp))
        return dict(box=box, skip=skip, leaf=leaf, order=order, rec=rec, rad=rad)

    def cast(self, P, V, bound=None):
        a = lambda x: np.ascontiguousarray(x, dtype=np.float32)
        P32, V32 = a(P), a(V)
        assert np.array_equal(P32.astype(float), P) and np.array_equal(V32.astype(float), V), "the rays are float32 numbers already"
        bd = a(np.full(len(P32), -1.0) if bound is None else bound)
        bvh = np.full(len(P32), 7.0, np.float32); brute = np.full(len(P32), 7.0, np.float32)
        self.lib.rth_cast(len(P32), P32.ctypes.data_as(self.fp), V32.ctypes.data_as(self.fp), bd.ctypes.data_as(self.fp), bvh.ctypes.data_as(self.fp), brute.ctypes.data_as(self.fp))
        return bvh, brute


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Host(hostbuild.shared(SRC, tmp_path_factory.mktemp("ray_tri_host")))


@pytest.fixture(scope="module")
def meshes(lib):
    """name -> triangles [nt, 3, 3] of the compiled model (the mesh's own frame): the shared meshes and PR2's asset with the most"""
    out = {name: rt.model_mesh_tris(rm.mesh_only_model(lib, *rt.MESHES[name]()))[0] for name in NAMES}
    assert [len(out[n]) for n in NAMES] == [576, 36, 72, 2, 12, 5]
    m = rm.load_robot(lib, "pr2")
    out["pr2 largest"] = rt.model_mesh_tris(m)[int(np.argmax(m.array("mesh_trinum")))]
    assert len(out["pr2 largest"]) >= 300
    return out


@pytest.mark.parametrize("name", NAMES + ["pr2 largest"])
def test_bvh_invariants(host, meshes, name):
    tris = meshes[name]
    B = host.build(tris)
    n, nt = len(B["skip"]), len(tris)
    skip, leaf, box = B["skip"], B["leaf"], B["box"]
    idx = np.arange(n)
    assert (idx < skip).all() and (skip <= n).all() and skip[0] == n
    is_leaf = leaf >= 0
    assert (skip[is_leaf] == idx[is_leaf] + 1).all()
    cnt, first = leaf[is_leaf] & 7, leaf[is_leaf] >> 3
    assert (cnt >= 1).all() and (cnt <= 4).all()
    assert np.array_equal(first, np.concatenate([[0], np.cumsum(cnt)[:-1]])) and cnt.sum() == nt, "leaves hold contiguous runs in leaf order: every record in exactly one leaf"
    assert sorted(B["order"]) == list(range(nt)), "every triangle once"
    if name == "flat_quad":
        assert n == 1 and leaf[0] == 2
    if name == "five":
        assert n == 3 and is_leaf.tolist() == [False, True, True]
    # preorder: the children of an inner node i are i + 1 and skip[i + 1], and the second one's subtree ends where i's does
    for i in idx[~is_leaf]:
        l, r = i + 1, skip[i + 1]
        assert r < skip[i] and skip[r] == skip[i]
        for c in (l, r):
            assert (box[c, :3] >= box[i, :3]).all() and (box[c, 3:] <= box[i, 3:]).all(), "a child's box lies inside its parent's"
    # a leaf's triangles (the fp64 corners and the stored fp32 record alike) lie inside its box
    rec = B["rec"]
    for i, f, c in zip(idx[is_leaf], first, cnt):
        for k in range(f, f + c):
            corners = tris[B["order"][k]]
            assert (corners >= box[i, :3]).all() and (corners <= box[i, 3:]).all()
            a, e1, e2 = rec[k, 0:3].astype(float), rec[k, 4:7].astype(float), rec[k, 8:11].astype(float)
            assert np.abs(a - corners[0]).max() <= 1e-7 * B["rad"][1] and np.abs(a + e1 - corners[1]).max() <= 2e-7 * B["rad"][1] and np.abs(a + e2 - corners[2]).max() <= 2e-7 * B["rad"][1]
            lo, hi = np.array([rec[k, 7], rec[k, 11], rec[k, 12]]), rec[k, 13:16]
            assert (corners >= lo).all() and (corners <= hi).all() and (lo >= box[i, :3]).all() and (hi <= box[i, 3:]).all()
    assert B["rad"][0] >= np.linalg.norm(tris.reshape(-1, 3), axis=1).max() and B["rad"][1] >= np.abs(tris.reshape(-1, 3)).sum(axis=1).max()


def _sets(name, tris):
    """(label, rays) of a mesh: two seeded general sets, the families of ray_mesh_ref (meshes whose corners span a volume; for the flat
    quad, which has no hull to take facets from, ray_tri_ref.planar_rays: in its plane and at its edges) and, for the torus, rays aimed
    exactly at float32-rounded vertices and edge midpoints"""
    out = [(f"set seed {s}", rt.mesh_ray_set(tris, NRAY, s)) for s in (11, 12)]
    if name != "flat_quad":
        pts = np.unique(tris.reshape(-1, 3), axis=0)
        for k, fam in enumerate(rm.MESH_FAMILIES):
            out.append((fam, rm.mesh_rays(pts, fam, 3.0, NRAY, seed=2000 + k)))
    else:
        out += [("in plane", rt.planar_rays(tris, "in plane", NRAY, 41)), ("at edges", rt.planar_rays(tris, "at edges", NRAY, 42))]
    if name == "torus":
        out += [("at vertices", rt.feature_rays(tris, "vertex", NRAY, 31)), ("at edge midpoints", rt.feature_rays(tris, "edge", NRAY, 32))]
    return out


@pytest.mark.parametrize("name", NAMES)
def test_ray_trimesh_against_the_loop_and_the_reference(host, meshes, name):
    tris = meshes[name]
    host.build(tris)
    scene = rt.tri_scene(tris)
    bad, shares = [], []
    for label, rays in _sets(name, tris):
        got, brute = host.cast(*rays)
        assert np.array_equal(got.view(np.uint32), brute.view(np.uint32)), (label, "pruning changed a result")
        # seeded with a nearer hit (three quarters of the ray's own) and with a farther one
        hitx = np.where(got >= 0, got, 1.0)
        for f in (0.75, 1.5):
            g2, b2 = host.cast(*rays, bound=(hitx * f).astype(np.float32))
            assert np.array_equal(g2.view(np.uint32), b2.view(np.uint32)), (label, f, "pruning changed a seeded result")
            if f < 1:
                assert (g2[got >= 0] == -1.0).all(), "nothing at or below a bound under the nearest hit"
            else:
                assert np.array_equal(g2[got >= 0], got[got >= 0])
        got = got.astype(float)
        ref, _ = rm.cast(rays[0], rays[1], scene)
        rob = rm.robust(rays, scene)
        hit = ref >= 0
        err = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        wrong = rob & (((got >= 0) != hit) | (hit & (err > TOL)))
        ok = rob & hit & (got >= 0)
        worst = float(err[ok].max()) if ok.any() else 0.0
        share = 1.0 - rob.mean()
        print(f"{name} {label}: {len(rob)} rays, non-robust share {share:.3f}, hits {int((rob & hit).sum())}, wrong {int(wrong.sum())}, max scaled error {worst:.3e}")
        shares.append((label, share))
        assert (got[~hit & rob] == -1.0).all(), label
        if label.startswith("at "):
            assert rob.mean() >= 0.9 and (got[rob] >= 0).all(), "watertight: a ray at a vertex or an edge does not pass between two triangles"
        if label == "at edges":
            assert (got[0::2] >= 0).all(), "every ray aimed at the edge the two triangles share hits"
        if wrong.any():
            bad.append((label, int(wrong.sum())))
    assert all(s <= 0.10 for _, s in shares), shares
    assert not bad, bad


def test_two_sided_inside_and_parallel(host, meshes):
    """box12 (half extents 0.2 / 0.15 / 0.1, its own frame is the box's up to a permutation of axes): from inside the far face, from
    outside the near one, a ray in the plane of a face misses that face (parallel) and takes the side it runs into"""
    tris = meshes["box12"]
    host.build(tris)
    half = np.abs(tris.reshape(-1, 3)).max(axis=0)
    ax = int(np.argmax(half))
    o = np.zeros(3); d = np.zeros(3); d[ax] = 1.0
    P = np.array([o + 0.05 * d, o - 1.0 * d, o + 1.0 * d, o - 1.0 * d], np.float32).astype(float)
    V = np.array([2.0 * d, 0.5 * d, d, -d], np.float32).astype(float)
    got, brute = host.cast(P, V)
    assert np.array_equal(got, brute)
    assert got[0] == pytest.approx((half[ax] - 0.05) / 2.0, abs=1e-6) and got[1] == pytest.approx((1.0 - half[ax]) / 0.5, abs=1e-6)
    assert got[2] == -1.0 and got[3] == -1.0
    k = (ax + 1) % 3
    Pp = o - 1.0 * d; Pp[k] = half[k]
    g, _ = host.cast(np.array([Pp], np.float32).astype(float), np.array([d], np.float32).astype(float))
    assert g[0] == pytest.approx(1.0 - half[ax], abs=1e-6), "in the plane of a face: the edge of the side it meets belongs to the mesh"


def test_sanitized_stand_alone_run_is_clean(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): BVHs of 1 .. 40 random triangles, of a
    576- and a 4800-triangle torus and of one triangle without area, the tables in exactly-sized heap arrays; every ray through the BVH
    and through the loop, fresh and seeded"""
    hostbuild.sanitized_run(SRC, "RAY_TRI_HOST_MAIN", tmp_path)
