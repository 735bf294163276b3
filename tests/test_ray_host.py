"""The ray kernel's own intersection code (csrc/dev_ray.h, __host__ __device__) on the CPU: tests/ray_host/ray_host.hip built as a
shared object and compared with the fp64 reference (ray_ref.geom_ray, which brute-forces every triangle of a height field and shares
nothing with the kernel's cell walk), and built as a stand-alone program with AddressSanitizer / UBSan on its host part.  No GPU.

On the rays the reference finds robust (ray_ref.robust): same hit / miss and |dist - ref| <= 5e-5 max(1, ref), the tolerance of
tests/test_gpu_ray.py.  The x86 build does not contract to FMA as the device build does: this is a rehearsal of the arithmetic and
of the control flow; the device figures are those of tests/test_gpu_ray.py.

Before the cell walk took its cell coordinates from one expression with a tolerance that grows with the grid (an absolute 1e-6
before), the height-field families failed here, wrong / robust rays: A nodes 21 / 266, A row planes 45 / 598, B nodes 42 / 266,
B column planes 91 / 598 (C and every other family 0) — every such ray through the terrain onto the base.  Since: 0 in every family,
worst scaled error 3.1e-6.

The second half casts world-frame rays through whole scenes with the code the ray and depth kernels share (ray_host_scene: the
verdict on a geom, the staged record, the walk; staged one record per geom as ray.hip does, and compacted as depth.hip does).
The frame composition (RAY_FRAME, through
ray_host_frame) is compared with numpy fp64.  The comparison of the casts is tests/ray_check.py's, the one of tests/test_gpu_depth.py."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import ray_mesh_ref as rm
import ray_ref as rr
from ray_check import check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "ray_host", "ray_host.hip")
TOL = 5e-5
PRIMS = [(rr.PLANE, (3.0, 2.0, 0.05))] + rr.PRIMITIVES
NAMES = {rr.PLANE: "plane", rr.SPHERE: "sphere", rr.CAPSULE: "capsule", rr.ELLIPSOID: "ellipsoid", rr.CYLINDER: "cylinder", rr.BOX: "box"}


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    """tests/ray_host/ray_host.hip as a shared object"""
    return C.CDLL(hostbuild.shared(SRC, tmp_path_factory.mktemp("ray_host")))


@pytest.fixture(scope="module")
def host(host_lib):
    lib = host_lib
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
    elevation array, border lines and corner nodes included, the primitive families, and the scene cast (1, 63, 64, 65 and 130
    geoms of every type over exactly-sized pose, size, ginfo, table and record arrays; every visibility rule; both staging orders)"""
    hostbuild.sanitized_run(SRC, "RAY_HOST_MAIN", tmp_path)


# ------------------------------------------------------------------ whole scenes through the kernels' shared code
class RayScene(C.Structure):      # csrc/dev_ray.h
    _fields_ = [("gpos", C.c_void_p), ("gmat", C.c_void_p), ("xpos", C.c_void_p), ("xquat", C.c_void_p), ("size", C.c_void_p), ("size_stride", C.c_longlong),
                ("slot_mask", C.c_void_p), ("sbase", C.c_int), ("ginfo", C.c_void_p), ("hf", C.c_void_p), ("hf_data", C.c_void_p), ("mesh", C.c_void_p),
                ("planes", C.c_void_p), ("env0", C.c_int), ("n", C.c_int), ("ngeom", C.c_int), ("nbody", C.c_int), ("bodyexclude", C.c_int),
                ("flg_static", C.c_int), ("cutoff", C.c_float)]


HF_DTYPE = np.dtype([("nrow", np.int32), ("ncol", np.int32), ("adr", np.int32), ("pad", np.int32), ("size", np.float32, 4)])      # RayHField
MESH_DTYPE = np.dtype([("adr", np.int32), ("num", np.int32), ("rbound", np.float32), ("pad", np.float32)])                           # RayMesh


def f32_scene(scene):
    """the scene with poses and sizes rounded to float32: the numbers the host code gets, so the reference works from the same ones"""
    return dict(scene, pos=rr.f32(scene["pos"]), mat=rr.f32(scene["mat"]), size=rr.f32(scene["size"]))


@pytest.fixture(scope="module")
def scene_cast(host_lib):
    lib = host_lib
    lib.ray_host_scene.argtypes = [C.POINTER(RayScene), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.ray_host_scene.restype = None
    off = (C.c_int * (len(RayScene._fields_) + 1))()
    lib.ray_host_scene_layout(off)      # the offset of every field, then the size
    assert list(off) == [getattr(RayScene, f).offset for f, _ in RayScene._fields_] + [C.sizeof(RayScene)], "the mirror of RayScene is out of date"

    def cast(scene, rays, compact, body=None, static=None, types=None, planes=None, slot_mask=None, sbase=0, env=0, bodyexclude=-1, flg_static=1):
        """(dist fp32, geomid) of float32 world-frame rays through `scene` (a ray_ref scene of float32 numbers).  body / static: per
        geom (default: body g + 1, not static); types: the ginfo types (default: the scene's); planes: {geom: [n, 4]} of its mesh geoms"""
        a = lambda x, t=np.float32: np.ascontiguousarray(x, dtype=t)
        ng = len(scene["type"])
        P, V = a(rays[0]), a(rays[1])
        assert np.array_equal(P.astype(float), rays[0]) and np.array_equal(V.astype(float), rays[1]), "the rays are float32 numbers already"
        gi = np.full((ng, 4), -1, np.int32)
        gi[:, 0] = scene["type"] if types is None else types
        gi[:, 1] = np.arange(1, ng + 1) if body is None else body
        gi[:, 2] = 0 if static is None else static
        hf = np.zeros(max(1, len(scene["hfield"])), HF_DTYPE); hd = []
        for k, (g, (nrow, ncol, hs, el)) in enumerate(sorted(scene["hfield"].items())):
            hf[k] = (nrow, ncol, sum(len(x) for x in hd), 0, hs); hd.append(a(el).ravel()); gi[g, 3] = k
        mesh = np.zeros(max(1, len(planes or {})), MESH_DTYPE); pl = []
        for k, (g, q) in enumerate(sorted((planes or {}).items())):
            q = np.vstack([q, np.tile([0.0, 0, 0, 1], ((-len(q)) % 4, 1))])      # (padded as the engine pads them)
            mesh[k] = (sum(len(x) for x in pl), len(q), np.sqrt((scene["mesh"][g].reshape(-1, 3) ** 2).sum(axis=1).max()), 0); pl.append(a(q)); gi[g, 3] = k
        hd = a(np.concatenate(hd) if hd else np.zeros(1)); pl = a(np.vstack(pl) if pl else np.zeros((1, 4)))
        pos, mat, size = a(scene["pos"]), a(scene["mat"]), a(scene["size"])
        assert np.array_equal(pos.astype(float), scene["pos"]) and np.array_equal(mat.astype(float), scene["mat"]) and np.array_equal(size.astype(float), scene["size"])
        sm = None if slot_mask is None else a(slot_mask, np.uint32)
        W = RayScene(gpos=pos.ctypes.data, gmat=mat.ctypes.data, size=size.ctypes.data, size_stride=0, slot_mask=None if sm is None else sm.ctypes.data, sbase=sbase,
                     ginfo=gi.ctypes.data, hf=hf.ctypes.data, hf_data=hd.ctypes.data, mesh=mesh.ctypes.data, planes=pl.ctypes.data, env0=env, n=1, ngeom=ng,
                     nbody=ng + 1, bodyexclude=bodyexclude, flg_static=flg_static, cutoff=0.0)
        dist = np.full(len(P), 7.0, np.float32); gid = np.full(len(P), 7, np.int32)
        lib.ray_host_scene(C.byref(W), int(compact), len(P), P.ctypes.data, V.ctypes.data, dist.ctypes.data, gid.ctypes.data)
        return dist, gid
    return cast


def both(scene_cast, scene, rays, **kw):
    """the cast staged as ray.hip stages and compacted as depth.hip compacts: the same bits"""
    d0, g0 = scene_cast(scene, rays, 0, **kw)
    d1, g1 = scene_cast(scene, rays, 1, **kw)
    assert np.array_equal(d0.view(np.uint32), d1.view(np.uint32)) and np.array_equal(g0, g1), "compacted and uncompacted staging give the same bits"
    return d0, g0


def test_scene_primitives_against_the_reference(scene_cast):
    """the plane and every primitive of ray_ref.PRIMITIVES (twice) at the poses of the GPU tests' primitives model"""
    scene = f32_scene(rr.scene_from_spec(rr.primitives_spec()))
    rays = rr.f32(*rr.primitive_rays(scene, 2000))
    dist, gid = both(scene_cast, scene, rays)
    check("primitives scene", dist, gid, scene, rays)
    assert {int(scene["type"][g]) for g in gid if g >= 0} == {rr.PLANE} | {t for t, _ in rr.PRIMITIVES}


def test_scene_hfield_and_mesh_against_the_reference(scene_cast, lib):
    """the table reads of the walk: the height field of the GPU tests and a tetrahedron mesh (its planes from the compiled model) over it"""
    m = rm.mesh_only_model(lib, rm.tetra_points())
    vert, planes = rm.model_mesh_verts(m)[0], rm.model_mesh_planes(m)[0]
    hs = rr.hfield_scene()
    q = np.array([0.8, -0.3, 0.4, 0.2]); q /= np.linalg.norm(q)
    scene = f32_scene(dict(pos=np.vstack([hs["pos"], [[0.2, -0.1, 1.3]], [[-0.9, 0.6, 1.1]]]), mat=np.vstack([hs["mat"], [rr.quat2mat(q)], [np.eye(3).ravel()]]),
                           size=np.vstack([hs["size"], np.zeros((1, 3)), [[0.2, 0, 0]]]), type=np.array([rr.HFIELD, rr.MESH, rr.SPHERE]), visible=np.ones(3, bool),
                           hfield=hs["hfield"]))
    scene["mesh"] = {1: rm.hull_triangles(vert)}
    rays = rr.f32(*rm.make_rays(7, scene, 1500, (-2.5, -2.5, -1.5), (2.5, 2.5, 2.5)))
    dist, gid = both(scene_cast, scene, rays, planes={1: planes})
    check("hfield + mesh scene", dist, gid, scene, rays)
    assert all((gid == g).sum() >= 50 for g in range(3)), "every geom is seen"
    # mesh mode 0: the mesh geom's ginfo type is -1 and the rays pass through it
    d0, g0 = both(scene_cast, scene, rays, types=[rr.HFIELD, -1, rr.SPHERE])
    check("hfield + hidden mesh", d0, g0, dict(scene, visible=np.array([True, False, True])), rays)
    assert not (g0 == 1).any()


@pytest.mark.parametrize("nsphere", [64, 65, 129, 130])
def test_scene_of_more_geoms_than_a_staging_pass(scene_cast, nsphere):
    """65 and 130 spheres over a floor (66 = 64 + 2 and 131 = 64 + 64 + 3 geoms), and 64 and 129 spheres, where the geoms number 65
    and 130: the pass boundary of RAY_PASS = 64 and a last partial pass of one, two and three records"""
    ngeom = nsphere + 1
    scene = f32_scene(rr.scene_from_spec(rr.many_spheres_spec(n=nsphere)))
    assert len(scene["type"]) == ngeom
    P, V = rr.many_spheres_rays(scene, nray=600)
    down = scene["pos"][1:] * [1, 1, 0] + [0, 0, 3.0]      # and straight down onto every sphere: each record of every pass is named
    rays = rr.f32(np.vstack([P, down]), np.vstack([V, np.tile([0, 0, -1.0], (nsphere, 1))]))
    dist, gid = both(scene_cast, scene, rays)
    check(f"{nsphere} spheres", dist, gid, scene, rays)
    assert np.array_equal(gid[600:], np.arange(1, ngeom))


def test_scene_visibility(scene_cast):
    """a hidden geom's id never comes back and the ray reports what lies behind it"""
    n = 70      # the pair under test sits behind the first pass boundary; the fillers are out of the rays' way
    pos = np.tile([0.0, 50.0, 0.0], (n, 1)); pos[66] = [1.0, 0, 0]; pos[68] = [3.0, 0, 0]
    scene = f32_scene(dict(pos=pos, mat=np.tile(np.eye(3).ravel(), (n, 1)), size=np.tile([0.2, 0, 0], (n, 1)), type=np.full(n, rr.SPHERE), visible=np.ones(n, bool), hfield={}))
    rays = rr.f32(np.array([[0.0, 0, 0], [0.0, 0.05, 0.02]]), np.array([[1.0, 0, 0], [2.0, 0, 0]]))
    body = np.arange(1, n + 1); static = np.zeros(n, int); static[66] = 1
    near, far = scene, dict(scene, visible=np.arange(n) != 66)
    mask = np.array([0, 1 << 3, 0], np.uint32)      # body sbase + 3 = geom 66's is inactive in env 1 only
    cases = [("all visible", {}, near), ("bodyexclude", dict(bodyexclude=67), far), ("flg_static 0", dict(flg_static=0), far),
             ("other body excluded", dict(bodyexclude=66), near), ("slot, env 1", dict(slot_mask=mask, sbase=64, env=1), far),
             ("slot, env 0", dict(slot_mask=mask, sbase=64, env=0), near), ("slot, env 2", dict(slot_mask=mask, sbase=64, env=2), near),
             ("ginfo type -1", dict(types=np.where(np.arange(n) == 66, -1, rr.SPHERE)), far)]
    for name, kw, ref in cases:
        dist, gid = both(scene_cast, scene, rays, body=body, static=static, **kw)
        check(name, dist, gid, ref, rays)
        assert (gid == (66 if ref is near else 68)).all(), name


def test_scene_tie_break(scene_cast):
    """two coincident geoms: the lower id, whether they share a pass or not, compacted or not"""
    n = 70
    pos = np.tile([0.0, 50.0, 0.0], (n, 1)); pos[[2, 5]] = [1.0, 0, 0]; pos[[7, 69]] = [0, 0, 2.0]
    scene = f32_scene(dict(pos=pos, mat=np.tile(np.eye(3).ravel(), (n, 1)), size=np.tile([0.2, 0.1, 0.15], (n, 1)), type=np.full(n, rr.BOX), visible=np.ones(n, bool), hfield={}))
    rays = rr.f32(np.array([[0.0, 0.01, 0.02], [0.03, 0.01, 0.0]]), np.array([[1.0, 0, 0], [0, 0, 1.5]]))
    dist, gid = both(scene_cast, scene, rays)
    assert gid.tolist() == [2, 7] and (dist > 0).all()
    dist2, gid2 = both(scene_cast, scene, rays, types=np.where(np.isin(np.arange(n), [2, 7]), -1, rr.BOX))
    assert gid2.tolist() == [5, 69] and np.array_equal(dist2.view(np.uint32), dist.view(np.uint32)), "the twin is at the same distance, bit for bit"


def test_frame_composition(host_lib):
    """RAY_FRAME (a site's or a camera's world pose from its body's) against a numpy fp64 composition of the same float32 inputs.
    Bound, from the fp32 roundings (u = 2^-24 each, written in units of 2^-23): a component of the product quaternion is a sum of four
    products of components below 1: off by at most 4 x 2^-23; an entry of S is quadratic in it (derivative at most 2 sum |s| <= 4)
    plus its own four roundings: 32 x 2^-23 in all.  A component of the origin is bp_k plus three products of entries of the body's
    matrix (each a few roundings of numbers below 1) with pos: 8 x 2^-23 x (|bp_k| + |pos|_1).  Measured: 1.02 and 1.91."""
    lib = host_lib
    lib.ray_host_frame.argtypes = [C.c_int] + [C.c_void_p] * 6
    lib.ray_host_frame.restype = None
    rng = np.random.default_rng(97)
    n = 1000
    unit = lambda q: q / np.linalg.norm(q, axis=1, keepdims=True)
    bp, bq = rng.uniform(-5, 5, (n, 3)), unit(rng.normal(size=(n, 4)))
    pos, quat = rng.uniform(-1, 1, (n, 3)), unit(rng.normal(size=(n, 4)))
    # directed: the identity frame in an unrotated body; a body turned by 180 degrees about z
    bp[0], bq[0], pos[0], quat[0] = (0.5, -1.5, 2.0), (1, 0, 0, 0), (0, 0, 0), (1, 0, 0, 0)
    bp[1], bq[1], pos[1], quat[1] = (0.5, -1.5, 2.0), (0, 0, 0, 1), (1, 2, 3), (1, 0, 0, 0)
    bp, bq, pos, quat = (np.ascontiguousarray(x, np.float32) for x in (bp, bq, pos, quat))
    o = np.zeros((n, 3), np.float32); S = np.zeros((n, 9), np.float32)
    lib.ray_host_frame(n, bp.ctypes.data, bq.ctypes.data, pos.ctypes.data, quat.ctypes.data, o.ctypes.data, S.ctypes.data)
    assert np.array_equal(o[0], bp[0]) and np.array_equal(S[0], np.eye(3, dtype=np.float32).ravel())
    assert np.array_equal(o[1], np.float32([-0.5, -3.5, 5.0])) and np.array_equal(S[1], np.float32([-1, 0, 0, 0, -1, 0, 0, 0, 1]))
    eps = 2.0 ** -23
    worst_o = worst_s = 0.0
    for i in range(n):
        B = rr.quat2mat(bq[i].astype(float)).reshape(3, 3)
        ref_o = bp[i].astype(float) + B @ pos[i].astype(float)
        ref_S = (B @ rr.quat2mat(quat[i].astype(float)).reshape(3, 3)).ravel()
        worst_o = max(worst_o, float((np.abs(o[i] - ref_o) / (np.abs(bp[i]) + np.abs(pos[i]).sum())).max()) / eps)
        worst_s = max(worst_s, float(np.abs(S[i] - ref_S).max()) / eps)
    print(f"frame composition, {n} poses: origin off by at most {worst_o:.2f} x 2^-23 (|bp_k| + |pos|_1) (bound 8), rotation by {worst_s:.2f} x 2^-23 (bound 32)")
    assert worst_o <= 8.0 and worst_s <= 32.0
