"""The shade kernel's own code (csrc/dev_render.h, __host__ __device__) on the CPU: tests/render_host/render_host.hip built as a shared
object — the depth kernel's cast, then a lane of mjh_shade_kernel per ray — against the fp64 reference tests/render_ref.py, by the
comparison of tests/render_check.py.  No GPU.

The scenes are the GPU tests' own models (built here through the same builder calls), at qpos0, with poses, sizes and rays rounded to
float32 so that the host code and the reference work from the same numbers.  The x86 build does not contract to FMA as the device
build does: a rehearsal of the arithmetic and of the control flow, and the measurement of N_HOST (render_check.py): the worst
max_c |n_host - n_ref| over the kept pixels of every image of IMAGES is asserted to be within the N_HOST written there.

Measured (`pytest tests/test_render_host.py -s` prints every case): see render_check.py's docstring for N_HOST and the excluded shares of
the images.  The directed ray sets stay under the same cap of 2 %: primitives from outside and inside (1940 rays) 0.0067 left out, worst
normal error 5.1e-6; the height field's directed and random rays (374) 0.0053, 1.0e-7; the meshes at 40 x 28, hulls and triangles,
0.0018, 1.2e-7; the flat panel's four rays 0."""
import ctypes as C
import os

import numpy as np
import pytest

import hostbuild
import ray_mesh_ref as rm
import ray_ref as rr
import render_check as rc
import render_ref as rf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "render_host", "render_host.hip")
TRIMESH = 8      # csrc/dev_ray.h: RAY_TYPE_TRIMESH


def f32_scene(scene):
    return dict(scene, pos=rr.f32(scene["pos"]), mat=rr.f32(scene["mat"]), size=rr.f32(scene["size"]))


class Host:
    def __init__(self, so):
        self.lib = C.CDLL(so)
        self.lib.render_host_image.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 8 + \
            [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float] + [C.c_void_p] * 5
        self.lib.render_host_image.restype = C.c_int
        self.lib.render_host_walk_pair.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        self.lib.render_host_walk_pair.restype = C.c_int

    def walk_pair(self, P, V, hfield=None, tris=None, bound=None):
        """(x of the instance without NRM, x of the one with it, the normal that one leaves [n, 3]) of geom-frame float32 rays through
        ray_hfield (hfield: elevations [nrow, ncol] and size[4]) or ray_trimesh (tris [nt, 3, 3]; bound per ray, default 3e38)"""
        a = lambda x, t=np.float32: np.ascontiguousarray(x, dtype=t)
        P, V = a(P), a(V)
        n = len(P)
        el, size = (a(hfield[0]), a(hfield[1])) if hfield is not None else (a(np.zeros((2, 2))), a(np.zeros(4)))
        t = a(tris if tris is not None else np.zeros((0, 3, 3)), np.float64)
        bd = a(np.full(n, 3e38) if bound is None else bound)
        x0 = np.full(n, 7.0, np.float32); x1 = np.full(n, 7.0, np.float32); nrm = np.full((n, 3), 7.0, np.float32)
        p = lambda x: x.ctypes.data
        assert self.lib.render_host_walk_pair(el.shape[0], el.shape[1], p(size), p(el), len(t), p(t), n, p(P), p(V), p(bd), p(x0), p(x1), p(nrm)) == 0
        return x0, x1, nrm

    def render(self, m, scene, rays, surface=None, range_=0, ambient=0.3, diffuse=0.7, background=(0.0, 0.0, 0.0, 0.0)):
        """(depth, gid, normal [n, 3], rgba uint8 [n, 4]) of float32 world-frame rays through model m posed as `scene` (float32 numbers);
        surface: None mesh geoms invisible, 0 their hulls, 1 their triangles"""
        a = lambda x, t=np.float32: np.ascontiguousarray(x, dtype=t)
        P, V = a(rays[0]), a(rays[1])
        assert np.array_equal(P.astype(float), rays[0]) and np.array_equal(V.astype(float), rays[1]), "the rays are float32 numbers already"
        ng = m.ngeom
        types, did = m.array("geom_type"), m.array("geom_dataid")
        nmesh, nhf = m.nmesh, m.nhfield
        pnum = m.array("mesh_planenum") if nmesh else np.zeros(0, np.int32)
        tnum = m.array("mesh_trinum") if nmesh else np.zeros(0, np.int32)
        gtype = np.array(types, np.int32); gdata = np.array(did, np.int32)
        for g in range(ng):
            if types[g] == rr.MESH:
                i = did[g]
                gtype[g] = -1 if surface is None else (TRIMESH if surface == 1 and tnum[i] > 0 else (rr.MESH if pnum[i] > 0 else -1))
            elif types[g] == rr.HFIELD and did[g] < 0:
                gtype[g] = -1
        hf_dim = a(np.stack([m.array("hfield_nrow"), m.array("hfield_ncol")], axis=1) if nhf else np.zeros((1, 2)), np.int32)
        hf_size = a(m.array("hfield_size") if nhf else np.zeros(4)); hf_adr = a(m.array("hfield_adr") if nhf else np.zeros(1), np.int32)
        hf_data = a(m.array("hfield_data") if nhf else np.zeros(1))
        verts = rm.model_mesh_verts(m) if nmesh else []
        rbound = a([np.sqrt((v ** 2).sum(axis=1).max()) if len(v) else 0.0 for v in verts] or [0.0])
        padr = a(m.array("mesh_planeadr") if nmesh else np.zeros(1), np.int32); pn = a(pnum if nmesh else np.zeros(1), np.int32)
        planes = a(m.array("mesh_plane") if len(m.array("mesh_plane")) else np.zeros(4))
        tadr = a(m.array("mesh_triadr") if nmesh else np.zeros(1), np.int32); tn = a(tnum if nmesh else np.zeros(1), np.int32)
        tris = a(m.array("mesh_tri") if m.nmeshtri else np.zeros(9), np.float64)
        pos, mat, size = a(scene["pos"]), a(scene["mat"]), a(scene["size"])
        assert np.array_equal(pos.astype(float), scene["pos"]) and np.array_equal(mat.astype(float), scene["mat"]) and np.array_equal(size.astype(float), scene["size"])
        col = a(rc.model_colours(m)); bg = a(background)
        n = len(P)
        depth = np.full(n, 7.0, np.float32); gid = np.full(n, 7, np.int32); nrm = np.full((n, 3), 7.0, np.float32); rgba = np.zeros(n, np.uint32)
        p = lambda x: x.ctypes.data
        r = self.lib.render_host_image(ng, p(pos), p(mat), p(size), p(gtype), p(gdata), nhf, p(hf_dim), p(hf_size), p(hf_adr), p(hf_data),
                                       nmesh, p(padr), p(pn), p(planes), p(rbound), p(tadr), p(tn), p(tris), p(col),
                                       n, p(P), p(V), int(range_), ambient, diffuse, p(bg), p(depth), p(gid), p(nrm), p(rgba))
        assert r == 0
        return depth, gid, nrm, rgba.view(np.uint8).reshape(n, 4)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return Host(hostbuild.shared(SRC, tmp_path_factory.mktemp("render_host")))


@pytest.fixture(scope="module")
def models(lib):
    out = dict(prim=rc.prim_model(lib, rig=True), spheres=rc.spheres_model(lib), hfield=rc.hfield_model(lib))
    out["meshes"], out["mesh_geoms"] = rc.meshes_model(lib)
    return out


def _scene(m, surface=None):
    return f32_scene(rc.model_scene(m, surface))


# ------------------------------------------------------------------ N_HOST and the excluded shares: the GPU tests' images
# (model, mesh surface, camera, width, height): every view and size tests/test_gpu_render.py renders, and the 64 x 48 views
IMAGES = [("prim", None, "front", 30, 20), ("prim", None, "front", 8, 8), ("prim", None, "front", 9, 8), ("prim", None, "front", 1, 1), ("prim", None, "front", 64, 48),
          ("prim", None, "side", 30, 20), ("prim", None, "side", 8, 8), ("prim", None, "side", 9, 8), ("prim", None, "side", 1, 1), ("prim", None, "side", 64, 48),
          ("prim", None, "eye", 30, 20), ("spheres", None, "above", 16, 16), ("hfield", None, "cam", 30, 20), ("hfield", None, "under", 30, 20),
          ("meshes", 0, "cam", 24, 16), ("meshes", 1, "cam", 24, 16)]


@pytest.mark.parametrize("name,surface,cam,width,height", IMAGES, ids=[f"{a}-{b}-{c}-{d}x{e}" for a, b, c, d, e in IMAGES])
def test_n_host_over_the_gpu_scenes(host, models, name, surface, cam, width, height):
    m = models[name]
    scene = _scene(m, surface)
    rays = rr.f32(*rc.model_camera_rays(m, m.name2id(5, cam), width, height))
    depth, gid, nrm, rgba = host.render(m, scene, rays, surface)
    worst_n, worst_c, share = rc.check_render(f"host {name} surface {surface} {cam} {width}x{height}", depth, gid, nrm, rgba, scene, rays,
                                              rc.model_colours(m), tol_n=rc.N_HOST)
    print(f"N_HOST candidate {worst_n:.3e}, excluded share {share:.4f}")
    if cam == "under":
        _, ref_g, _, feat = rf.cast(rays[0], rays[1], scene)
        assert ((ref_g == 0) & (feat == -1) & (gid == 0)).sum() > 50 and ((ref_g == 0) & (feat <= -2)).sum() > 20, "the base and a wall are in view"
    if name == "prim" and cam == "eye":
        rigg = m.name2id(2, "rigg")
        assert (gid == rigg).all(), "the camera sits inside its body's ball"
        c = scene["pos"][rigg]
        inward = (c - (rays[0] + depth[:, None].astype(float) * rays[1])) / rc.RIG_RADIUS
        assert np.abs(nrm - inward).max() < 1e-4, "from inside a sphere the normal points at its centre"


# ------------------------------------------------------------------ directed cases
def test_every_primitive_from_outside_and_inside(host, models):
    m = models["prim"]
    scene = _scene(m)
    P, V = rr.primitive_rays(scene, 1500)
    rng = np.random.default_rng(3)
    solid = [g for g in range(m.ngeom) if scene["type"][g] != rr.PLANE]
    Pi = np.vstack([scene["pos"][g] + rng.uniform(-0.03, 0.03, size=(40, 3)) for g in solid])
    Vi = rng.normal(size=(len(Pi), 3)); Vi *= rng.uniform(0.5, 2.0, size=(len(Pi), 1)) / np.linalg.norm(Vi, axis=1, keepdims=True)
    rays = rr.f32(np.vstack([P, Pi]), np.vstack([V, Vi]))
    depth, gid, nrm, rgba = host.render(m, scene, rays)
    rc.check_render("host primitives, random rays", depth, gid, nrm, rgba, scene, rays, rc.model_colours(m))
    inside = gid[len(P):]
    assert np.array_equal(inside, np.repeat(solid, 40)), "a ray from a geom's centre hits that geom's far surface"
    assert {int(scene["type"][g]) for g in gid[:len(P)] if g >= 0} == {rr.PLANE} | {t for t, _ in rr.PRIMITIVES}
    # from inside the normal points back in: against the ray, towards the half space the origin is in
    assert (np.sum(nrm[len(P):] * rays[1][len(P):], axis=1) < 0).all()


def test_height_field_top_wall_and_base(host, models):
    m = models["hfield"]
    scene = _scene(m)
    rays = rr.f32(*rr.hfield_rays(scene, nrand=600))
    # (without the rays that end on the model's far body, a 5 cm ball 50 m up: its normal is an fp32 hit point 50 m away over 0.05)
    near = rf.cast(rays[0], rays[1], scene)[1] <= 0
    rays = (rays[0][near], rays[1][near])
    depth, gid, nrm, rgba = host.render(m, scene, rays)
    rc.check_render("host height field, directed and random rays", depth, gid, nrm, rgba, scene, rays, rc.model_colours(m))
    _, ref_g, _, feat = rf.cast(rays[0], rays[1], scene)
    f = feat[ref_g == 0]
    assert (f == -1).any() and (f <= -2).any(), "the base and a wall are seen"
    tri = f[f >= 0]
    both = {c for c in set(tri // 2) if (2 * c in tri) and (2 * c + 1 in tri)}
    assert both, "both triangles of a cell are seen"


def test_hull_and_triangles_of_a_non_convex_mesh(host, models):
    m, (g_torus, g_jaw, g_quad) = models["meshes"], models["mesh_geoms"]
    cam = m.name2id(5, "cam")
    rays = rr.f32(*rc.model_camera_rays(m, cam, 40, 28))
    out = {}
    for surface in (0, 1):
        scene = _scene(m, surface)
        depth, gid, nrm, rgba = host.render(m, scene, rays, surface)
        rc.check_render(f"host meshes, surface {surface}", depth, gid, nrm, rgba, scene, rays, rc.model_colours(m))
        out[surface] = (gid, nrm)
    through = (out[1][0] == 0) & (out[0][0] == g_torus)
    assert through.any(), "the triangles let the camera see the floor through the torus's hole, which the hull fills"
    assert np.abs(out[1][1][through] - [0.0, 0.0, 1.0]).max() < 1e-6, "there the normal is the floor's"
    assert np.abs(out[0][1][through] - out[1][1][through]).max() > 1e-3, "and the hull's differs"
    assert (out[1][0] == g_quad).any() and not (out[0][0] == g_quad).any(), "a mesh without volume has no hull"


def test_flat_panel_from_both_sides(host, models):
    m, (_, _, g_quad) = models["meshes"], models["mesh_geoms"]
    scene = _scene(m, 1)
    c = scene["pos"][g_quad]
    P = np.array([c + [0.02, 0.01, 1.0], c + [0.02, 0.01, -0.5], c + [-0.05, 0.03, 0.7], c + [-0.05, 0.03, -0.6]])
    V = np.array([[0, 0, -1.0], [0, 0, 1.0], [0.05, 0, -1.0], [0.0, -0.04, 0.8]])
    rays = rr.f32(P, V)
    depth, gid, nrm, rgba = host.render(m, scene, rays, 1)
    rc.check_render("host flat panel", depth, gid, nrm, rgba, scene, rays, rc.model_colours(m))
    assert (gid == g_quad).all()
    R = scene["mat"][g_quad].reshape(3, 3)
    up = R[:, np.argmax(np.abs(R.T @ nrm[0].astype(float)))]      # the panel's normal axis in the world
    assert np.abs(np.abs(nrm.astype(float) @ up) - 1.0).max() < 1e-5
    assert np.sign(nrm[0] @ up) == -np.sign(nrm[1] @ up) and np.sign(nrm[2] @ up) == -np.sign(nrm[3] @ up), "each side sees the normal that faces it"


def test_flat_shade_is_exact_and_the_background_is_kept(host, models):
    m = models["prim"]
    scene = _scene(m)
    rays = rr.f32(*rc.model_camera_rays(m, 0, 30, 20))
    bg = (0.2, 0.4, 0.6, 1.0)
    depth, gid, nrm, rgba = host.render(m, scene, rays, ambient=1.0, diffuse=0.0, background=bg)
    assert (gid < 0).any() and (gid >= 0).any()
    assert np.array_equal(rgba, rc.flat_colours(rc.model_colours(m), gid, bg))
    # range = 1: the ray parameter is recovered from the distance; normals and colours stay within the tolerance
    d1, g1, n1, c1 = host.render(m, scene, rays, range_=1)
    rc.check_render("host primitives front, range 1", d1, g1, n1, c1, scene, rays, rc.model_colours(m), scale=np.linalg.norm(rays[1], axis=1))


# ------------------------------------------------------------------ one walk, two instances (csrc/dev_ray.h: ray_hfield<NRM>, ray_trimesh<NRM>)
def _pair_rays(rng, lo, hi, inside, n):
    """n geom-frame rays from around the box [lo, hi] aimed into it, n from the points `inside` (a random direction each)"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    c, r = 0.5 * (lo + hi), np.linalg.norm(hi - lo)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    P = c + u * rng.uniform(0.8, 3.0, size=(n, 1)) * r
    V = (rng.uniform(lo - 0.1 * r, hi + 0.1 * r, size=(n, 3)) - P) * rng.uniform(0.3, 2.0, size=(n, 1))
    Pi = np.asarray(inside, float)[rng.integers(0, len(inside), n)]
    Vi = rng.normal(size=(n, 3))
    return np.vstack([P, Pi]), np.vstack([V, Vi])


def _same_walk(x0, x1, nrm, what):
    assert x0.tobytes() == x1.tobytes(), f"{what}: the instance with NRM returns other bits"
    assert np.array_equal(np.abs(nrm).max(axis=1) > 0, x1 >= 0), f"{what}: a non-zero normal exactly where there is a hit"
    assert (x1 >= 0).sum() > len(x1) // 4 and (x1 < 0).sum() > 20, f"{what}: hits and misses both occur"


@pytest.mark.parametrize("nrow,ncol", [(2, 2), (3, 4)])
def test_hfield_walk_with_normal_is_the_walk_without(host, nrow, ncol):
    """2 x 2: one cell — both triangles, four walls, the base; 3 x 4: strips and rows to walk.  Rays from outside, from inside the solid,
    and on and along grid lines (column lines, row lines, the cells' diagonals)"""
    rng = np.random.default_rng(100 * nrow + ncol)
    size = np.array([0.6, 0.4, 0.3, 0.1], np.float32)
    el = rng.uniform(0.2, 1.0, size=(nrow, ncol)).astype(np.float32)
    sx, sy, sz, sb = size.astype(float)
    inside = rng.uniform([-sx, -sy, -sb], [sx, sy, 0.2 * sz], size=(50, 3))      # below the lowest elevation: in the solid
    P, V = _pair_rays(rng, [-sx, -sy, -sb], [sx, sy, sz], inside, 600)
    # grid lines: origins on a line x = column / y = row (exact in the grid's own units for these sizes or not: both kinds occur), the
    # direction within the line's vertical plane; the diagonal of a cell, seen from above and from below
    xs, ys = np.linspace(-sx, sx, ncol), np.linspace(-sy, sy, nrow)
    Pl, Vl = [], []
    for k in range(300):
        up = 1.0 if k % 2 else -1.0
        x, y = xs[rng.integers(ncol)], ys[rng.integers(nrow)]
        t = rng.uniform(-1.2, 1.2)
        Pl += [[x, t * sy, -up * 1.0], [t * sx, y, -up * 1.0], [x, y, -up * 1.0]]
        Vl += [[0.0, rng.uniform(-0.5, 0.5), up], [rng.uniform(-0.5, 0.5), 0.0, up], [0.0, 0.0, up]]
        a, b = rng.uniform(-1.0, 2.0, 2)      # two points of the diagonal u = w of cell (0, 0), continued beyond it
        dx, dy = 2 * sx / (ncol - 1), 2 * sy / (nrow - 1)
        Pl.append([-sx + a * dx, -sy + a * dy, -up * 1.0]); Vl.append([(b - a) * dx, (b - a) * dy, up * 2.0])
    rays = rr.f32(np.vstack([P, Pl]), np.vstack([V, Vl]))
    x0, x1, nrm = host.walk_pair(rays[0], rays[1], hfield=(el, size))
    _same_walk(x0, x1, nrm, f"height field {nrow} x {ncol}")
    hit = nrm[x1 >= 0]
    axes = {tuple(r) for r in hit[hit[:, 2] != 1.0].astype(int)}
    assert axes == {(0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0)}, "the base and the four walls give hits"
    tops = {tuple(r) for r in hit[hit[:, 2] == 1.0]}
    assert len(tops) == 2 * (nrow - 1) * (ncol - 1), "and so does every top triangle"


def _tetra():
    c = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], float) * 0.3
    return np.array([[c[j] for j in range(4) if j != k] for k in range(4)])


def _box12():
    h = np.array([0.5, 0.3, 0.2])
    c = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * h
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return np.array([[c[q[0]], c[q[i]], c[q[i + 1]]] for q in quads for i in (1, 2)])


@pytest.mark.parametrize("name", ["tetrahedron", "box12"])
def test_trimesh_walk_with_normal_is_the_walk_without(host, name):
    """a tetrahedron: one leaf; a box of 12 triangles: four leaves under inner nodes with a skip.  Rays from outside, from inside the
    solid, and at the corners and edge midpoints; unbounded, then with the bound a little above the hit (render_normal's)"""
    rng = np.random.default_rng(len(name))
    tris = _tetra() if name == "tetrahedron" else _box12()
    corners = tris.reshape(-1, 3)
    lo, hi = corners.min(axis=0), corners.max(axis=0)
    P, V = _pair_rays(rng, lo, hi, rng.uniform(-0.02, 0.02, size=(50, 3)), 800)
    aim = np.vstack([corners, 0.5 * (tris + np.roll(tris, 1, axis=1)).reshape(-1, 3)])      # shared vertices and edges
    Pa = rng.normal(size=(len(aim), 3)) * 1.5
    rays = rr.f32(np.vstack([P, Pa]), np.vstack([V, aim - Pa]))
    x0, x1, nrm = host.walk_pair(rays[0], rays[1], tris=tris)
    _same_walk(x0, x1, nrm, name)
    assert (x1[800:1600] >= 0).all(), "from inside a closed mesh every ray hits"
    bound = np.where(x1 >= 0, x1 + np.float32(1e-3) * np.abs(x1) + np.float32(1e-30), np.float32(3e38)).astype(np.float32)
    b0, b1, bn = host.walk_pair(rays[0], rays[1], tris=tris, bound=bound)
    _same_walk(b0, b1, bn, name + ", bounded")
    assert b1.tobytes() == x1.tobytes() and bn.tobytes() == nrm.tobytes(), "the bound above the hit prunes nothing the scan would take"
    # e1 x e2 of one of the mesh's triangles, and of one the hit point lies in the plane of
    N = np.cross(tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0])
    h = x1 >= 0
    X = rays[0][h] + x1[h, None].astype(float) * rays[1][h]
    for n, x in zip(nrm[h].astype(float), X):
        k = np.argmin(np.abs(N - n).max(axis=1))
        assert np.abs(N[k] - n).max() < 1e-6 and abs(N[k] @ (x - tris[k, 0])) < 1e-5 * np.linalg.norm(N[k])


def test_sanitized_stand_alone_run_is_clean(tmp_path):
    """the same source with its own main under AddressSanitizer / UBSan (host part only): random scenes of 1 .. 130 geoms of every type,
    hulls and triangle meshes included, over exactly-sized arrays; rays from outside and from inside the geoms; every hit a unit normal
    that faces its ray, every miss the zero normal and the background"""
    hostbuild.sanitized_run(SRC, "RENDER_HOST_MAIN", tmp_path)
