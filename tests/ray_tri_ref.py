"""Small non-convex meshes, ray sets and model helpers for the tests of rays against a mesh's OWN triangles (mjh_ray_set_mesh_surface 1).

The fp64 reference is the one the project has, ray_mesh_ref.tri_ray / cast / robust: it is fed the model's mesh_tri through
ray_mesh_ref.attach_meshes(scene, m, model_mesh_tris(m)) instead of scipy's hull triangles.  numpy only.

Every generator returns (vert [nv, 3], face [nf, 3] int32).  A compiled model holds the triangles in the mesh's own frame (centre of mass,
principal axes): ray sets are made from model_mesh_tris(m), not from the generators' coordinates."""
import numpy as np

import ray_mesh_ref as rm
import ray_ref as rr


# ------------------------------------------------------------------ meshes
def torus(R=0.3, r=0.1, nu=24, nv=12):
    """closed, 2 nu nv triangles (576), axis z: a hole the hull fills"""
    u = 2 * np.pi * np.arange(nu) / nu; v = 2 * np.pi * np.arange(nv) / nv
    U, V = np.meshgrid(u, v, indexing="ij")
    vert = np.stack([(R + r * np.cos(V)) * np.cos(U), (R + r * np.cos(V)) * np.sin(U), r * np.sin(V)], axis=-1).reshape(-1, 3)
    face = []
    for i in range(nu):
        for j in range(nv):
            a, b, c, d = i * nv + j, ((i + 1) % nu) * nv + j, ((i + 1) % nu) * nv + (j + 1) % nv, i * nv + (j + 1) % nv
            face += [(a, b, c), (a, c, d)]
    return vert, np.array(face, np.int32)


_QUADS = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward, corners indexed x y z (bits 4 2 1)


def _box(lo, hi):
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    vert = np.array([[(lo, hi)[x][0], (lo, hi)[y][1], (lo, hi)[z][2]] for x in (0, 1) for y in (0, 1) for z in (0, 1)])
    face = [t for q in _QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return vert, np.array(face, np.int32)


JAW_BOXES = [((-0.2, -0.2, -0.05), (-0.1, 0.2, 0.05)),       # the back plate
             ((-0.1, 0.12, -0.05), (0.25, 0.2, 0.05)),       # two fingers
             ((-0.1, -0.2, -0.05), (0.25, -0.12, 0.05))]


def jaw():
    """36 triangles: a U of three touching boxes, interior faces included (as CAD exports have them)"""
    vs, fs, n = [], [], 0
    for lo, hi in JAW_BOXES:
        v, f = _box(lo, hi)
        vs.append(v); fs.append(f + n); n += len(v)
    return np.vstack(vs), np.vstack(fs).astype(np.int32)


def sheet(n=6):
    """2 n^2 triangles (72): an open wavy surface z = 0.05 sin 7x cos 5y over [-0.3, 0.3]^2"""
    g = np.linspace(-0.3, 0.3, n + 1)
    X, Y = np.meshgrid(g, g, indexing="ij")
    vert = np.stack([X, Y, 0.05 * np.sin(7 * X) * np.cos(5 * Y)], axis=-1).reshape(-1, 3)
    face = []
    for i in range(n):
        for j in range(n):
            a, b, c, d = i * (n + 1) + j, (i + 1) * (n + 1) + j, (i + 1) * (n + 1) + j + 1, i * (n + 1) + j + 1
            face += [(a, b, c), (a, c, d)]
    return vert, np.array(face, np.int32)


def flat_quad():
    """4 vertices, 2 triangles, no volume: no hull planes, so invisible as a hull; its BVH is a single leaf root"""
    vert = np.array([[-0.2, -0.15, 0.0], [0.2, -0.15, 0.0], [0.2, 0.15, 0.0], [-0.2, 0.15, 0.0]])
    return vert, np.array([(0, 1, 2), (0, 2, 3)], np.int32)


def box12():
    """ray_mesh_ref.box_points() with its 12 faces"""
    face = [t for q in _QUADS for t in ((q[0], q[1], q[2]), (q[0], q[2], q[3]))]
    return rm.box_points(), np.array(face, np.int32)


def five():
    """5 triangles: an open pentagonal pyramid (a BVH root with two leaves)"""
    a = 2 * np.pi * np.arange(5) / 5
    vert = np.vstack([[[0.0, 0.0, 0.2]], np.stack([0.25 * np.cos(a), 0.25 * np.sin(a), -0.05 + 0.02 * np.arange(5)], axis=1)])
    return vert, np.array([(0, 1 + k, 1 + (k + 1) % 5) for k in range(5)], np.int32)


MESHES = {"torus": torus, "jaw": jaw, "sheet": sheet, "flat_quad": flat_quad, "box12": box12, "five": five}


# ------------------------------------------------------------------ models
def model_mesh_tris(m):
    """the triangles of every mesh asset of a model: list of [ntri, 3, 3] (a, b, c) in the frame of mesh_vert"""
    adr, num, t = m.array("mesh_triadr"), m.array("mesh_trinum"), m.array("mesh_tri").reshape(-1, 3, 3)
    return [t[adr[i]:adr[i] + num[i]] for i in range(len(adr))]


def tri_scene(tris):
    """one mesh geom alone, unrotated at the world origin: the world frame is the geom's"""
    return dict(pos=np.zeros((1, 3)), mat=np.eye(3).reshape(1, 9), size=np.zeros((1, 3)), type=np.array([rr.MESH]), visible=np.ones(1, bool),
                hfield={}, mesh={0: np.asarray(tris, float)})


def add_mesh(lib, b, vert, face):
    import ctypes as C
    v = np.ascontiguousarray(vert, float); f = np.ascontiguousarray(face, np.int32)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), f.ctypes.data_as(C.POINTER(C.c_int)), len(f), None)
    assert mid >= 0, lib.mjh_last_error()
    return mid


def scene_model(lib, items, floor=True, camera=None, primitives=False, site=None):
    """a floor plane (static, geom 0) and one mesh geom per item: (mesh name or (vert, face), pos, quat or None, free) — free: on a free
    body of its own, else a static geom of the world; items with the same mesh name share one asset.  camera: (pos, quat, fovy) of a
    camera fixed in the world.  primitives: ray_mesh_ref._add_primitives first (then no separate floor: they bring a bounded one).
    site: (item index, pos, quat) a site on that item's body.  -> (model, geom ids of the items, body ids (0: static))"""
    import mujoco_sim_amd as ms
    from helpers import D, set_opt
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=[0, 0, 0])
    if primitives:
        rm._add_primitives(lib, b, D)
    elif floor:
        assert lib.mjh_builder_add_geom(b, b"floor", 0, rr.PLANE, D(0.0, 0.0, 0.05), D(0, 0, 0), None, None, -1, -1, -1, -1) >= 0
    assets, bodies = {}, []
    for k, (mesh, pos, quat, free) in enumerate(items):
        key = mesh if isinstance(mesh, str) else id(mesh)
        if key not in assets:
            assets[key] = add_mesh(lib, b, *(MESHES[mesh]() if isinstance(mesh, str) else mesh))
        q = None if quat is None else D(*quat)
        if free:
            bd = lib.mjh_builder_add_body(b, b"mb%d" % k, 0, D(*pos), q, 0.0)
            lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
            assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, bd, assets[key], None, None, None, -1, -1, -1, -1) >= 0
        else:
            bd = 0
            assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, 0, assets[key], D(*pos), q, None, -1, 0, 0, -1) >= 0
        bodies.append(bd)
    if site is not None:
        assert lib.mjh_builder_add_site(b, b"scanner", bodies[site[0]], D(*site[1]), D(*site[2])) >= 0
    if camera is not None:
        assert lib.mjh_builder_add_camera(b, b"cam", 0, D(*camera[0]), D(*camera[1]), float(camera[2])) >= 0
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m, [m.name2id(2, "mg%d" % k) for k in range(len(items))], bodies


# ------------------------------------------------------------------ ray sets in the frame of one mesh (rounded to float32)
def mesh_ray_set(tris, nray, seed):
    """three quarters of the origins 1 .. 3 m out, aimed at a point within 1.25 bounding radii of the origin of the frame; a fifth inside
    the bounding sphere, any direction; the rest out there and pointing away.  Directions of length 0.5 .. 2."""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tris, float)
    rad = float(np.linalg.norm(tris.reshape(-1, 3), axis=1).max())

    def unit(n):
        u = rng.normal(size=(n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True)
    n_in, n_away = nray // 5, nray // 20
    n_out = nray - n_in - n_away
    T = unit(n_out) * 1.25 * rad * rng.uniform(size=(n_out, 1)) ** (1 / 3)
    P_out = unit(n_out) * (rad + rng.uniform(1.0, 3.0, size=(n_out, 1)))
    P_in = unit(n_in) * rad * rng.uniform(size=(n_in, 1)) ** (1 / 3)
    P_aw = unit(n_away) * (rad + rng.uniform(1.0, 3.0, size=(n_away, 1)))
    P = np.vstack([P_out, P_in, P_aw])
    V = np.vstack([T - P_out, unit(n_in), P_aw])
    V = V / np.linalg.norm(V, axis=1, keepdims=True) * rng.uniform(0.5, 2.0, size=(nray, 1))
    return rr.f32(P, V)


def feature_rays(tris, kind, nray, seed, dist=2.0):
    """rays from outside aimed EXACTLY at float32-rounded vertices ("vertex") or at float32-rounded edge midpoints ("edge") of a closed
    mesh, from the side of the surface normal (within 30 degrees of it): the watertightness check"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tris, float)
    k = rng.integers(len(tris), size=nray)
    c = rng.integers(3, size=nray)
    a, b = tris[k, c], tris[k, (c + 1) % 3]
    T = rr.f32(a if kind == "vertex" else 0.5 * (a + b))
    n = np.cross(tris[k, 1] - tris[k, 0], tris[k, 2] - tris[k, 0])
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    u = rng.normal(size=(nray, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = n + 0.5 * u; u /= np.linalg.norm(u, axis=1, keepdims=True)
    P = rr.f32(T + dist * u)
    return P, rr.f32(T - P)


def planar_rays(tris, kind, nray, seed, dist=3.0):
    """ray families for a flat mesh (flat_quad: no hull, so ray_mesh_ref.mesh_rays has no facets to aim at).  "in plane": a direction
    within the mesh's plane across a point of the mesh, the origin lifted off the plane by +-1 % of the extent (one in 25 not lifted
    at all: grazing, never robust — they exercise the parallel test).  "at edges": half of the rays aimed exactly at float32-rounded
    points of an edge two triangles share (they must hit: the mesh is watertight there), half at points of an outer edge moved 2 % of the
    extent towards the centroid; from either side of the plane, within 60 degrees of its normal"""
    rng = np.random.default_rng(seed)
    tris = np.asarray(tris, float)
    pts = tris.reshape(-1, 3)
    n = np.cross(tris[0, 1] - tris[0, 0], tris[0, 2] - tris[0, 0]); n /= np.linalg.norm(n)
    cen = pts.mean(axis=0)
    ext = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    k = rng.integers(len(tris), size=nray)
    if kind == "in plane":
        w = rng.dirichlet(np.ones(3) * 2.0, size=nray)
        T = np.einsum("ij,ijk->ik", w, tris[k])
        e = tris[0, 1] - tris[0, 0]; e /= np.linalg.norm(e)
        f = np.cross(n, e)
        a = rng.uniform(0, 2 * np.pi, size=(nray, 1))
        u = np.cos(a) * e + np.sin(a) * f
        lift = rng.choice([-1.0, 1.0], size=(nray, 1)) * 0.01 * ext
        lift[: nray // 25] = 0.0
        T = T + lift * n
        P = rr.f32(T - dist * u)
        V = T - P
        return P, rr.f32(V * (rng.uniform(0.5, 2.0, size=(nray, 1)) / np.linalg.norm(V, axis=1, keepdims=True)))
    edges = {}
    for t in tris:
        for c in range(3):
            key = tuple(sorted((tuple(np.round(t[c], 12)), tuple(np.round(t[(c + 1) % 3], 12)))))
            edges.setdefault(key, []).append((t[c], t[(c + 1) % 3]))
    shared = [v[0] for v in edges.values() if len(v) == 2]
    outer = [v[0] for v in edges.values() if len(v) == 1]
    assert shared and outer
    s = rng.uniform(0.05, 0.95, size=(nray, 1))
    T = np.zeros((nray, 3))
    for i in range(nray):
        a, b = (shared if i % 2 == 0 else outer)[rng.integers(len(shared if i % 2 == 0 else outer))]
        T[i] = a + s[i] * (b - a)
        if i % 2:
            T[i] += 0.02 * ext * (cen - T[i]) / np.linalg.norm(cen - T[i])
    T = rr.f32(T)
    u = rng.normal(size=(nray, 3)); u /= np.linalg.norm(u, axis=1, keepdims=True)
    u = rng.choice([-1.0, 1.0], size=(nray, 1)) * n + 0.8 * u; u /= np.linalg.norm(u, axis=1, keepdims=True)
    P = rr.f32(T + dist * u)
    return P, rr.f32(T - P)
