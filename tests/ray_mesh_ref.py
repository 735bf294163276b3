"""fp64 numpy reference for rays against mesh geoms (mjh_ray in mesh mode 1) and the meshes / ray sets the mesh ray tests share.

A mesh geom is the convex hull of its kept vertices (the model's mesh_vert, in the geom's own frame).  The reference builds that hull
with scipy.spatial.ConvexHull and intersects rays with the hull's TRIANGLES, two-sided, taking the nearest x >= 0: it shares neither the
model builder's hull nor the kernel's half-space clipping.  A triangle includes its edges with an absolute slack of 1e-12 in its
barycentric coordinates (as ray_ref's height-field triangles do), so a ray through an edge cannot fall between two neighbours.

A scene is a ray_ref scene with one more entry, "mesh": {geom: triangles [nt, 3, 3] in the geom's frame}.  cast() merges the mesh hits
with ray_ref.cast (every other geom type) by the smaller distance; robust() is ray_ref.robust's rule on the merged result: same geom and
a distance within 1e-3 under 1e-4 shifts of the origin.

hull_inside() / march() are the independent method for the reference itself: march the point-membership test (all hull inequalities
<= 0) along the ray and bisect the first change."""
import numpy as np

import ray_ref as rr

EDGE_SLACK = 1e-12


# ------------------------------------------------------------------ the shared test meshes
BOX_HALF = np.array([0.2, 0.15, 0.1])      # the box of ray_ref.mesh_model


def box_points():
    """(a) the box of ray_ref.mesh_model: 8 corner points"""
    return np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * BOX_HALF


def tetra_points():
    """(b) an irregular tetrahedron"""
    return np.array([[0.25, 0.0, -0.1], [-0.15, 0.2, -0.1], [-0.15, -0.2, -0.12], [0.02, 0.01, 0.22]])


ELLIPSOID_AXES = np.array([0.3, 0.2, 0.15])


def ellipsoid_points(seed=3, n=20):
    """(c) n seeded points on an ellipsoid with semi-axes 0.3 / 0.2 / 0.15: every one a hull vertex, every facet a generic triangle"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True) * ELLIPSOID_AXES


def box_stl_points():
    """(d) that box as 12 triangles with repeated vertices (36 of them, as an STL file lists them), then the 6 face centres and the 12 edge
    midpoints: (vert [54, 3], face [12, 3])"""
    c = box_points()
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]      # outward, corners indexed x y z (bits 4 2 1)
    tri = []
    for q in quads:
        tri += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    vert = np.array([c[i] for t in tri for i in t])
    face = np.arange(36, dtype=np.int32).reshape(12, 3)
    centres = np.array([s * BOX_HALF[k] * np.eye(3)[k] for k in range(3) for s in (-1, 1)])
    mids = np.array([(c[i] + c[j]) / 2 for i in range(8) for j in range(i + 1, 8) if bin(i ^ j).count("1") == 1])
    assert len(mids) == 12
    return np.vstack([vert, centres, mids]), face


# ------------------------------------------------------------------ models
ROBOT_FILES = {"pr2": "pr2/pr2.xml", "hsrb4s": "hsrb4s/hsrb4s.xml", "tiago": "tiago/tiago.xml", "armar6": "armar/armar6.xml"}


def mesh_only_model(lib, vert, face=None):
    """one free body carrying one mesh geom built from the given points (and triangles)"""
    import ctypes as C

    import mujoco_sim_amd as ms
    from helpers import D
    b = lib.mjh_builder_create()
    v = np.ascontiguousarray(vert, float)
    f = None if face is None else np.ascontiguousarray(face, np.int32)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None if f is None else f.ctypes.data_as(C.POINTER(C.c_int)),
                                   0 if f is None else len(f), None)
    assert mid >= 0, lib.mjh_last_error()
    bd = lib.mjh_builder_add_body(b, b"m", 0, D(0, 0, 1.0), None, 0.0)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    assert lib.mjh_builder_add_mesh_geom(b, b"mg", bd, mid, None, None, None, -1, -1, -1, -1) >= 0
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m


def load_robot(lib, name, world=False):
    """a bundled robot with its mesh assets through the MJCF loader (refmodels.model_dir()); world: on the world file's floor"""
    import os

    import mujoco_sim_amd as ms
    from refmodels import model_dir
    ref = os.path.join(model_dir(), "test")
    paths = ([os.path.join(ref, "..", "world", "empty.xml")] if world else []) + [os.path.join(ref, ROBOT_FILES[name])]
    lib.mjh_load_set_bounds(1e-6, 1e-6); lib.mjh_load_set_mesh_mode(1)      # (as the robot fixtures are compiled)
    try:
        m = ms.load_mjcf(paths=paths)
    finally:
        lib.mjh_load_set_bounds(0.0, 0.0)
    # ... with the contact / row capacity of the bundled fixture of the same model (tests/golden/make_robot_fixtures.py sets it the same
    # way): the loader's default capacity is more than an engine takes for a model of this size
    fixture = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"robot_{name}{'_world' if world else ''}_mesh.npz")
    if os.path.exists(fixture):
        z = np.load(fixture)
        m.c.maxcon = int(z["int__maxcon"]); m.c.maxefc = int(z["int__maxefc"])
    return m


# ------------------------------------------------------------------ hull, triangles, rays
def hull_of(vert):
    from scipy.spatial import ConvexHull
    return ConvexHull(np.asarray(vert, float).reshape(-1, 3))


def hull_triangles(vert):
    """triangles [nt, 3, 3] of the convex hull of the points (scipy / qhull)"""
    h = hull_of(vert)
    return h.points[h.simplices]


def tri_ray(P, V, tris):
    """nearest x >= 0 with P + x V on one of the triangles (either side), -1: none.  P, V: [N, 3]"""
    P = np.asarray(P, float).reshape(-1, 3); V = np.asarray(V, float).reshape(-1, 3)
    best = np.full(len(P), -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        for a, b, c in tris:
            e1, e2 = b - a, c - a
            n = np.cross(e1, e2)
            x = ((a - P) @ n) / (V @ n)
            x = np.where(np.isfinite(x), x, -1.0)
            Q = P + x[:, None] * V - a
            d11, d12, d22 = e1 @ e1, e1 @ e2, e2 @ e2
            q1, q2 = Q @ e1, Q @ e2
            det = d11 * d22 - d12 * d12
            b1, b2 = (d22 * q1 - d12 * q2) / det, (d11 * q2 - d12 * q1) / det
            ok = (x >= 0) & (b1 >= -EDGE_SLACK) & (b2 >= -EDGE_SLACK) & (b1 + b2 <= 1 + EDGE_SLACK)
            best = np.where(ok & ((best < 0) | (x < best)), x, best)
    return best


def cast(pnt, vec, scene, cutoff=0.0):
    """(dist, geomid) of world-frame rays against every visible geom of the scene, mesh geoms (scene["mesh"]) included"""
    P = np.asarray(pnt, float).reshape(-1, 3); V = np.asarray(vec, float).reshape(-1, 3)
    best, gid = rr.cast(P, V, scene)      # (without a cutoff: it applies to the merged result)
    for g, tris in scene.get("mesh", {}).items():
        if not scene["visible"][g]:
            continue
        R = np.asarray(scene["mat"][g], float).reshape(3, 3)
        x = tri_ray((P - scene["pos"][g]) @ R, V @ R, tris)
        take = (x >= 0) & ((gid < 0) | (x < best))
        best = np.where(take, x, best); gid = np.where(take, g, gid)
    if cutoff > 0:
        far = best > cutoff
        best = np.where(far, -1.0, best); gid = np.where(far, -1, gid)
    return best, gid.astype(np.int32)


def robust(rays, scene, shift=1e-4, tol=1e-3):
    """ray_ref.robust's rule on the merged result"""
    P = np.asarray(rays[0], float).reshape(-1, 3); V = np.asarray(rays[1], float).reshape(-1, 3)
    d0, g0 = cast(P, V, scene)
    u = V / np.linalg.norm(V, axis=1, keepdims=True)
    helper = np.where(np.abs(u[:, [0]]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    e1 = np.cross(u, helper); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(u, e1)
    ok = np.ones(len(P), bool)
    for e in (e1, e2):
        for s in (shift, -shift):
            d, g = cast(P + s * e, V, scene)
            ok &= (g == g0) & (np.abs(d - d0) <= tol)
    return ok


def single_mesh_scene(vert):
    """one mesh geom alone, unrotated at the world origin: the world frame is the geom's"""
    return dict(pos=np.zeros((1, 3)), mat=np.eye(3).reshape(1, 9), size=np.zeros((1, 3)), type=np.array([rr.MESH]), visible=np.ones(1, bool),
                hfield={}, mesh={0: hull_triangles(vert)})


def model_mesh_verts(m):
    """the kept vertices of every mesh asset of a model: list of [nvert, 3]"""
    adr, num, v = m.array("mesh_vertadr"), m.array("mesh_vertnum"), m.array("mesh_vert").reshape(-1, 3)
    return [v[adr[i]:adr[i] + num[i]] for i in range(len(adr))]


def model_mesh_planes(m):
    """the hull planes of every mesh asset of a model: list of [nplane, 4] (n, d)"""
    adr, num, p = m.array("mesh_planeadr"), m.array("mesh_planenum"), m.array("mesh_plane").reshape(-1, 4)
    return [p[adr[i]:adr[i] + num[i]] for i in range(len(adr))]


def attach_meshes(scene, m, tris_by_mesh=None):
    """scene["mesh"] for every mesh geom of model m (triangles per mesh asset computed once and shared); returns the scene"""
    if tris_by_mesh is None:
        tris_by_mesh = [hull_triangles(v) for v in model_mesh_verts(m)]
    types, did = m.array("geom_type"), m.array("geom_dataid")
    scene["mesh"] = {int(g): tris_by_mesh[did[g]] for g in np.nonzero(types == rr.MESH)[0]}
    return scene


# ------------------------------------------------------------------ independent method: march the membership test
def hull_inside(X, equations, margin=0.0):
    """bool [N]: all hull inequalities n.x + b <= margin (scipy's ConvexHull.equations)"""
    X = np.asarray(X, float).reshape(-1, 3)
    return (X @ equations[:, :3].T + equations[:, 3] <= margin).all(axis=1)


def march(P, V, equations, length=8.0, step=1e-3, tol=1e-9):
    """distance (units of |V|) to the first change of hull_inside along each ray, -1 if there is none within `length` metres"""
    P = np.asarray(P, float).reshape(-1, 3); V = np.asarray(V, float).reshape(-1, 3)
    nv = np.linalg.norm(V, axis=1)
    U = V / nv[:, None]
    out = np.full(len(P), -1.0)
    ts = np.arange(0.0, length + step, step)
    for i in range(len(P)):
        ins = hull_inside(P[i] + ts[:, None] * U[i], equations)
        k = np.nonzero(ins[1:] != ins[:-1])[0]
        if len(k) == 0:
            continue
        lo, hi, a = ts[k[0]], ts[k[0] + 1], ins[k[0]]
        while hi - lo > tol:
            mid = 0.5 * (lo + hi)
            if hull_inside(P[i] + mid * U[i], equations)[0] == a: lo = mid
            else: hi = mid
        out[i] = 0.5 * (lo + hi) / nv[i]
    return out


# ------------------------------------------------------------------ ray sets in the frame of one mesh (rounded to float32)
def fibonacci(n):
    i = np.arange(n)
    z = 1 - 2 * (i + 0.5) / n
    r = np.sqrt(1 - z * z); ph = i * 2.399963229728653
    return np.stack([r * np.cos(ph), r * np.sin(ph), z], axis=1)


MESH_FAMILIES = ["random", "inside", "face normal", "in face plane", "through edge", "through vertex"]


def mesh_rays(vert, family, dist, nray, seed):
    """rays in the frame of one mesh, origins `dist` metres from their target (inside: origins within the hull), rounded to float32.
    random: aimed at a point inside the hull; inside: from a point inside, any direction; face normal: along -n onto a point of a facet
    (vec is the rounded normal itself); in face plane: a direction within a facet's plane, the origin lifted off the plane by +-1 % of
    the extent (half of them pass above the facet, half below it through the solid; one in 25 is not lifted at all); through edge / through vertex: aimed at the midpoint
    of a hull edge / at a hull vertex from outside, then moved 2 % of the extent towards the centroid so that the ray enters the solid"""
    rng = np.random.default_rng(seed)
    h = hull_of(vert)
    pts = h.points
    cen = pts[h.vertices].mean(axis=0)
    ext = float(np.linalg.norm(pts.max(axis=0) - pts.min(axis=0)))
    tris = pts[h.simplices]

    def interior(n):
        w = rng.dirichlet(np.ones(len(h.vertices)), size=n)
        return cen + 0.8 * (w @ pts[h.vertices] - cen)

    def unit(n):
        u = rng.normal(size=(n, 3))
        return u / np.linalg.norm(u, axis=1, keepdims=True)
    ln = rng.uniform(0.5, 2.0, size=(nray, 1))
    if family == "random":
        T = interior(nray); P = T + dist * unit(nray)
    elif family == "inside":
        P = interior(nray); T = P + unit(nray)
    elif family in ("face normal", "in face plane"):
        k = rng.integers(len(tris), size=nray)
        w = rng.dirichlet(np.ones(3) * 2.0, size=nray)
        T = np.einsum("ij,ijk->ik", w, tris[k])
        n = h.equations[k, :3]
        if family == "face normal":
            P = T + dist * n
        else:
            e = tris[k, 1] - tris[k, 0]; e /= np.linalg.norm(e, axis=1, keepdims=True)
            f = np.cross(n, e)
            a = rng.uniform(0, 2 * np.pi, size=(nray, 1))
            u = np.cos(a) * e + np.sin(a) * f
            lift = rng.choice([-1.0, 1.0], size=(nray, 1)) * 0.01 * ext
            lift[: nray // 25] = 0.0      # (one in 25 exactly in the facet's plane: grazing, so never robust — they exercise den == 0)
            T = T + lift * n
            P = T - dist * u
    else:
        if family == "through edge":
            ed = {tuple(sorted((s[i], s[(i + 1) % 3]))) for s in h.simplices for i in range(3)}
            ed = np.array(sorted(ed))
            k = rng.integers(len(ed), size=nray)
            T = 0.5 * (pts[ed[k, 0]] + pts[ed[k, 1]])
        else:
            T = pts[h.vertices[rng.integers(len(h.vertices), size=nray)]]
        out = T - cen
        out /= np.linalg.norm(out, axis=1, keepdims=True)
        u = unit(nray)
        u = np.where((np.sum(u * out, axis=1) < 0)[:, None], -u, u)      # from outside
        u = u + 0.5 * out; u /= np.linalg.norm(u, axis=1, keepdims=True)
        T = T + 0.02 * ext * (cen - T) / np.linalg.norm(cen - T, axis=1, keepdims=True)
        P = T + dist * u
    P = rr.f32(P)
    V = T - P
    V = rr.f32(V * (ln / np.linalg.norm(V, axis=1, keepdims=True)))
    return P, V


# ------------------------------------------------------------------ world-frame ray sets over scenes with meshes
def geom_radius(scene, g):
    """bounding radius of geom g about its frame origin (a plane / height field: 0)"""
    t = int(scene["type"][g])
    if t == rr.MESH:
        return float(np.linalg.norm(scene["mesh"][g].reshape(-1, 3), axis=1).max())
    return rr.rbound(t, scene["size"][g])


def make_rays(seed, scene, nray, origin_lo, origin_hi, miss_share=0.2, miss_lift=1.0):
    """ray_ref.make_rays with mesh geoms among the targets: origins uniform in the box outside every solid's bounding sphere (and above
    a plane), each aimed at a point within half the bounding radius of a random visible geom (a plane: a point of its footprint),
    directions of length 0.5 .. 2; a fixed share points away from the scene and up"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(origin_lo, float), np.asarray(origin_hi, float)
    ng = len(scene["type"])
    rad = np.array([geom_radius(scene, g) for g in range(ng)])
    solid = [g for g in range(ng) if rad[g] > 0]
    P = np.zeros((0, 3))
    while len(P) < nray:
        X = rng.uniform(lo, hi, size=(4 * nray, 3))
        ok = np.ones(len(X), bool)
        for g in solid:
            ok &= np.linalg.norm(X - scene["pos"][g], axis=1) > rad[g] * 1.05
        P = np.vstack([P, X[ok]])
    P = P[:nray]
    targets = [g for g in range(ng) if scene["visible"][g] and int(scene["type"][g]) != rr.HFIELD]
    V = np.zeros((nray, 3))
    nmiss = int(round(miss_share * nray))
    for i in range(nray):
        if i >= nray - nmiss:
            d = P[i] - scene["pos"][targets].mean(axis=0)
            d[2] = abs(d[2]) + miss_lift
        else:
            g = targets[rng.integers(len(targets))]
            R = scene["mat"][g].reshape(3, 3); s = scene["size"][g]
            if int(scene["type"][g]) == rr.PLANE:
                ex = [s[0] if s[0] > 0 else 1.0, s[1] if s[1] > 0 else 1.0]
                loc = np.array([rng.uniform(-ex[0], ex[0]), rng.uniform(-ex[1], ex[1]), 0.0])
            else:
                u = rng.normal(size=3); u /= np.linalg.norm(u)
                loc = u * 0.5 * rad[g] * rng.uniform() ** (1 / 3)
            d = scene["pos"][g] + R @ loc - P[i]
        V[i] = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
    return rr.f32(P, V)


def tetra_field_spec(nmesh=70, nsphere=35, seed=47):
    """more static geoms than one staging pass of the kernel holds (64): nmesh small tetrahedron-mesh geoms (ONE asset: tetra_points()
    scaled by 0.4) and nsphere spheres, interleaved on a grid over a floor.  list of dicts (type, size, pos, quat), type MESH for the
    mesh geoms"""
    rng = np.random.default_rng(seed)
    spec = [dict(type=rr.PLANE, size=(0.0, 0.0, 0.05), pos=(0.0, 0.0, 0.0), quat=(1.0, 0, 0, 0))]
    n = nmesh + nsphere
    for k in range(n):
        i, j = k % 10, k // 10
        pos = (0.45 * (i - 4.5), 0.45 * (j - 5.0), rng.uniform(0.3, 1.2))
        if k % 3 == 2 and sum(s["type"] == rr.SPHERE for s in spec) < nsphere:
            spec.append(dict(type=rr.SPHERE, size=(rng.uniform(0.06, 0.1), 0, 0), pos=pos, quat=(1.0, 0, 0, 0)))
        else:
            spec.append(dict(type=rr.MESH, size=(0.0, 0, 0), pos=pos, quat=tuple(rr.random_quat(rng))))
    return spec


def pr2_fan(nx=16, nz=8):
    """nx * nz rays from a scanner 2 m in front of the PR2 (which stands at the origin facing +x) at chest height (1.0 m), looking back at
    it: azimuth +-13 degrees about -x, elevation -27 .. +8 degrees"""
    az = np.deg2rad(np.linspace(-13.0, 13.0, nx) + 0.37)
    el = np.deg2rad(np.linspace(-27.0, 8.0, nz) + 0.21)
    A, E = np.meshgrid(az, el)
    V = np.stack([-np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=-1).reshape(-1, 3)
    P = np.tile([2.0, 0.0, 1.0], (len(V), 1))
    return rr.f32(P, V)


# ------------------------------------------------------------------ models of the device tests
MIXED_MESH_POS = [(-0.9, 1.35, 1.0), (0.0, 1.35, 0.9), (0.9, 1.35, 1.1)]
MIXED_STATIC_POS, MIXED_STATIC_QUAT = (1.8, 1.35, 0.6), tuple(np.array([0.8, -0.3, 0.4, 0.2]) / np.linalg.norm([0.8, -0.3, 0.4, 0.2]))
MIXED_SITE_POS, MIXED_SITE_QUAT = (0.3, 0.05, 0.1), tuple(np.array([0.7, 0.1, -0.5, 0.3]) / np.linalg.norm([0.7, 0.1, -0.5, 0.3]))


def _add_mesh(lib, b, pts):
    import ctypes as C
    v = np.ascontiguousarray(pts, float)
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    assert mid >= 0, lib.mjh_last_error()
    return mid


def primitives_model(lib):
    """ray_ref.primitives_spec() alone: a model without meshes"""
    import mujoco_sim_amd as ms
    from helpers import D, set_opt
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=[0, 0, 0])
    _add_primitives(lib, b, D)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    return m


def _add_primitives(lib, b, D):
    for k, g in enumerate(rr.primitives_spec()):
        if g["free"]:
            bd = lib.mjh_builder_add_body(b, b"free%d" % k, 0, D(*g["pos"]), D(*g["quat"]), 0.0)
            lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, bd, g["type"], D(*g["size"]), None, None, None, -1, -1, -1, -1) >= 0
        else:
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, -1, -1, -1) >= 0


def mixed_model(lib):
    """ray_ref.primitives_spec() (a bounded floor, every primitive once static and once on a free body) plus the meshes (a), (b), (c) on
    a free body each, the tetrahedron once more as a static geom, and a site on (a)'s body.
    -> (model, mesh body ids [3], site id)"""
    import mujoco_sim_amd as ms
    from helpers import D, set_opt
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, gravity=[0, 0, 0])
    _add_primitives(lib, b, D)
    mids = [_add_mesh(lib, b, pts) for pts in (box_points(), tetra_points(), ellipsoid_points())]
    bodies = []
    for k, mid in enumerate(mids):
        bd = lib.mjh_builder_add_body(b, b"mesh%d" % k, 0, D(*MIXED_MESH_POS[k]), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, bd, mid, None, None, None, -1, -1, -1, -1) >= 0
        bodies.append(bd)
    assert lib.mjh_builder_add_mesh_geom(b, b"mstatic", 0, mids[1], D(*MIXED_STATIC_POS), D(*MIXED_STATIC_QUAT), None, -1, -1, -1, -1) >= 0
    site = lib.mjh_builder_add_site(b, b"scanner", bodies[0], D(*MIXED_SITE_POS), D(*MIXED_SITE_QUAT))
    assert site >= 0
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m, bodies, site


def mixed_qpos(m, nenv, seed=17):
    """a qpos per env: every free body moved by up to 0.1 m per axis and turned to a random orientation"""
    rng = np.random.default_rng(seed)
    q = np.tile(m.array("qpos0"), (nenv, 1))
    for i in range(nenv):
        for k in range(m.nq // 7):
            q[i, 7 * k:7 * k + 3] += rng.uniform(-0.1, 0.1, size=3)
            q[i, 7 * k + 3:7 * k + 7] = rr.random_quat(rng)
    return q


MIXED_ORIGIN_LO, MIXED_ORIGIN_HI = (-3.0, -2.0, 0.05), (3.0, 2.2, 3.0)


def tetra_field_model(lib):
    """tetra_field_spec() as a model: every geom static, one mesh asset shared by the 70 mesh geoms, plus a far moving body"""
    import mujoco_sim_amd as ms
    from helpers import D, set_opt
    spec = tetra_field_spec()
    b = lib.mjh_builder_create()
    set_opt(lib, b, gravity=[0, 0, 0])
    mid = _add_mesh(lib, b, 0.4 * tetra_points())
    for k, g in enumerate(spec):
        if g["type"] == rr.MESH:
            assert lib.mjh_builder_add_mesh_geom(b, b"g%d" % k, 0, mid, D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
        else:
            assert lib.mjh_builder_add_geom(b, b"g%d" % k, 0, g["type"], D(*g["size"]), D(*g["pos"]), D(*g["quat"]), None, -1, 0, 0, -1) >= 0
    bd = lib.mjh_builder_add_body(b, b"far", 0, D(0, 0, 50.0), None, 0.0)
    lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"fg", bd, rr.SPHERE, D(0.05, 0, 0), None, None, None, -1, 0, 0, -1)
    p = lib.mjh_builder_compile(b)
    assert p, lib.mjh_last_error()
    m = ms.Model(p, lib)
    lib.mjh_builder_destroy(b)
    return m, spec


def oracle_scene(m, qpos=None, tris_by_mesh=None):
    """the scene of a model at qpos (default qpos0) from the fp64 oracle's kinematics: the CPU stand-in for the device's geom poses"""
    import orc
    d = orc.OrcData(m.ptr)
    if qpos is not None:
        d.f("qpos")[:] = qpos
    d.call("kinematics")
    sc = rr.scene_from_device(d.f("geom_xpos").copy(), d.f("geom_xmat").copy(), m.array("geom_size"), m.array("geom_type"))
    return attach_meshes(sc, m, tris_by_mesh)
