"""fp64 numpy reference for batched ray casting (mjh_ray: mj_ray's semantics) and the scenes / ray sets the ray tests use.

A scene is a dict of arrays: pos [ng, 3], mat [ng, 9] (row-major, world = R local), size [ng, 3], type [ng], visible [ng] (bool)
and hfield {geom: (nrow, ncol, size[4], data[nrow, ncol])}.  cast() returns (dist, geomid): the smallest x >= 0 with
pnt + x vec on the surface of a visible geom (in units of |vec|) and that geom; a miss is (-1, -1).

Geoms: a plane is hit on its front (+z) face only and bounded by size[0], size[1] where those are > 0; sphere, capsule,
ellipsoid, cylinder (flat caps) and box at the nearest non-negative root (an origin inside hits the far surface); a height
field is the solid the collision code uses — two triangles per cell sharing the diagonal (r, c)-(r+1, c+1), side walls and base
down to -size[3] — hit at its nearest surface from any side (a triangle includes its edges with an absolute slack of 1e-12 in its
barycentric coordinates, so a ray that lies on a grid line cannot fall between two neighbours); meshes are invisible.

robust() marks the rays whose result does not flip under a 1e-4 shift of the origin: grazing and edge rays change geom or
jump in distance on fp32 rounding, and no tolerance on the device result is meaningful for them.

inside() / march() are an independent method (no formula shared with the closed forms): march the point-membership test
along the ray in steps of 1e-3 and bisect the first change to 1e-9."""
import numpy as np

PLANE, HFIELD, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = range(8)


# ------------------------------------------------------------------ closed forms (geom frame; P, V: [N, 3])
def _pick(best, x, ok=True):
    take = ok & (x >= 0) & ((best < 0) | (x < best))
    return np.where(take, x, best)


def _quad_roots(P, V, r, dims):
    """both roots of |P + x V|^2 = r^2 over the coordinates `dims`, NaN where there is none"""
    a = np.sum(V[:, dims] ** 2, axis=1)
    b = np.sum(V[:, dims] * P[:, dims], axis=1)
    c = np.sum(P[:, dims] ** 2, axis=1) - r * r
    with np.errstate(invalid="ignore", divide="ignore"):
        disc = b * b - a * c
        s = np.sqrt(np.where(disc >= 0, disc, np.nan))
        x0, x1 = (-b - s) / a, (-b + s) / a
    bad = ~(a > 0)
    return np.where(bad, np.nan, x0), np.where(bad, np.nan, x1)


def _plane(P, V, s):
    with np.errstate(invalid="ignore", divide="ignore"):
        x = -P[:, 2] / V[:, 2]
    ok = (V[:, 2] < 0) & (x >= 0)
    H = P + np.where(ok, x, 0.0)[:, None] * V
    if s[0] > 0:
        ok &= np.abs(H[:, 0]) <= s[0]
    if s[1] > 0:
        ok &= np.abs(H[:, 1]) <= s[1]
    return np.where(ok, x, -1.0)


def _sphere(P, V, r):
    best = np.full(len(P), -1.0)
    for x in _quad_roots(P, V, r, [0, 1, 2]):
        best = _pick(best, np.nan_to_num(x, nan=-1.0))
    return best


def _ellipsoid(P, V, s):
    return _sphere(P / s, V / s, 1.0)


def _side(P, V, r, half, best):
    for x in _quad_roots(P, V, r, [0, 1]):
        xx = np.nan_to_num(x, nan=-1.0)
        best = _pick(best, xx, np.abs(P[:, 2] + xx * V[:, 2]) <= half)
    return best


def _capsule(P, V, s):
    best = _side(P, V, s[0], s[1], np.full(len(P), -1.0))
    for sg in (1.0, -1.0):
        Pc = P - np.array([0, 0, sg * s[1]])
        for x in _quad_roots(Pc, V, s[0], [0, 1, 2]):
            xx = np.nan_to_num(x, nan=-1.0)
            best = _pick(best, xx, sg * (Pc[:, 2] + xx * V[:, 2]) >= 0)
    return best


def _cylinder(P, V, s):
    best = _side(P, V, s[0], s[1], np.full(len(P), -1.0))
    for z in (s[1], -s[1]):
        with np.errstate(invalid="ignore", divide="ignore"):
            x = (z - P[:, 2]) / V[:, 2]
        x = np.where(np.isfinite(x), x, -1.0)
        H = P + x[:, None] * V
        best = _pick(best, x, H[:, 0] ** 2 + H[:, 1] ** 2 <= s[0] ** 2)
    return best


def _slabs(P, V, lo, hi):
    with np.errstate(invalid="ignore", divide="ignore"):
        a, b = (lo - P) / V, (hi - P) / V
    par = V == 0
    t0 = np.where(par, -np.inf, np.minimum(a, b)).max(axis=1)
    t1 = np.where(par, np.inf, np.maximum(a, b)).min(axis=1)
    out = (par & ((P < lo) | (P > hi))).any(axis=1)
    return t0, t1, (t0 <= t1) & ~out


def _box(P, V, s):
    t0, t1, ok = _slabs(P, V, -np.asarray(s), np.asarray(s))
    ok &= t1 >= 0
    return np.where(ok, np.where(t0 >= 0, t0, t1), -1.0)


def hfield_height(hf, x, y):
    """terrain height over (x, y) of the hfield frame (inside the footprint), by the cell's two triangles"""
    nrow, ncol, size, data = hf
    fx = np.clip((x + size[0]) / (2 * size[0]) * (ncol - 1), 0, ncol - 1)
    fy = np.clip((y + size[1]) / (2 * size[1]) * (nrow - 1), 0, nrow - 1)
    c = np.minimum(fx.astype(int), ncol - 2); r = np.minimum(fy.astype(int), nrow - 2)
    u, w = fx - c, fy - r
    z = np.asarray(data) * size[2]
    z00, z01, z10, z11 = z[r, c], z[r, c + 1], z[r + 1, c], z[r + 1, c + 1]
    return np.where(u >= w, z00 + u * (z01 - z00) + w * (z11 - z01), z00 + w * (z10 - z00) + u * (z11 - z10))


EDGE_SLACK = 1e-12


def _hfield(P, V, hf):
    nrow, ncol, size, data = hf
    sx, sy, sz, sb = size
    best = np.full(len(P), -1.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        # base
        x = (-sb - P[:, 2]) / V[:, 2]
        x = np.where(np.isfinite(x), x, -1.0)
        H = P + x[:, None] * V
        best = _pick(best, x, (np.abs(H[:, 0]) <= sx) & (np.abs(H[:, 1]) <= sy))
        # walls below the terrain's edge
        for ax, sa, so in ((0, sx, sy), (1, sy, sx)):
            for w in (-1.0, 1.0):
                x = (w * sa - P[:, ax]) / V[:, ax]
                x = np.where(np.isfinite(x), x, -1.0)
                H = P + x[:, None] * V
                H[:, ax] = w * sa
                ok = (np.abs(H[:, 1 - ax]) <= so) & (H[:, 2] >= -sb) & (H[:, 2] <= hfield_height(hf, H[:, 0], H[:, 1]))
                best = _pick(best, x, ok)
        # top triangles: every cell, both triangles, as planes through three vertices (barycentric inclusion)
        z = np.asarray(data) * sz
        xs = -sx + 2 * sx * np.arange(ncol) / (ncol - 1); ys = -sy + 2 * sy * np.arange(nrow) / (nrow - 1)
        for r in range(nrow - 1):
            for c in range(ncol - 1):
                a = np.array([xs[c], ys[r], z[r, c]]); d = np.array([xs[c + 1], ys[r + 1], z[r + 1, c + 1]])
                for third in (np.array([xs[c + 1], ys[r], z[r, c + 1]]), np.array([xs[c], ys[r + 1], z[r + 1, c]])):
                    e1, e2 = d - a, third - a
                    n = np.cross(e1, e2)
                    den = V @ n
                    x = ((a - P) @ n) / den
                    x = np.where(np.isfinite(x), x, -1.0)
                    Q = P + x[:, None] * V - a
                    # barycentric coordinates in the triangle's plane
                    d11, d12, d22 = e1 @ e1, e1 @ e2, e2 @ e2
                    q1, q2 = Q @ e1, Q @ e2
                    det = d11 * d22 - d12 * d12
                    b1, b2 = (d22 * q1 - d12 * q2) / det, (d11 * q2 - d12 * q1) / det
                    # (absolute slack: a ray exactly on an edge may miss both neighbours by one fp64 rounding; the terrain is
                    #  continuous, so taking the neighbour's plane at its edge changes no distance)
                    best = _pick(best, x, (b1 >= -EDGE_SLACK) & (b2 >= -EDGE_SLACK) & (b1 + b2 <= 1 + EDGE_SLACK))
    return best


def geom_ray(gtype, P, V, size, hf=None):
    """closed-form distances of rays (P, V) given in the frame of one geom; -1: miss"""
    P = np.asarray(P, float).reshape(-1, 3); V = np.asarray(V, float).reshape(-1, 3)
    if gtype == PLANE: return _plane(P, V, size)
    if gtype == SPHERE: return _sphere(P, V, size[0])
    if gtype == CAPSULE: return _capsule(P, V, size)
    if gtype == ELLIPSOID: return _ellipsoid(P, V, np.asarray(size, float))
    if gtype == CYLINDER: return _cylinder(P, V, size)
    if gtype == BOX: return _box(P, V, size)
    if gtype == HFIELD and hf is not None: return _hfield(P, V, hf)
    return np.full(len(P), -1.0)


def cast(pnt, vec, scene, cutoff=0.0):
    """(dist [nray], geomid [nray]) of world-frame rays against every visible geom of a scene"""
    P = np.asarray(pnt, float).reshape(-1, 3); V = np.asarray(vec, float).reshape(-1, 3)
    best = np.full(len(P), -1.0); gid = np.full(len(P), -1, dtype=np.int32)
    for g in range(len(scene["type"])):
        t = int(scene["type"][g])
        if not scene["visible"][g] or t == MESH or (t == HFIELD and g not in scene.get("hfield", {})):
            continue
        R = np.asarray(scene["mat"][g], float).reshape(3, 3)
        lp = (P - scene["pos"][g]) @ R; lv = V @ R
        x = geom_ray(t, lp, lv, scene["size"][g], scene.get("hfield", {}).get(g))
        take = (x >= 0) & ((gid < 0) | (x < best))
        best = np.where(take, x, best); gid = np.where(take, g, gid)
    if cutoff > 0:
        far = best > cutoff
        best = np.where(far, -1.0, best); gid = np.where(far, -1, gid)
    return best, gid.astype(np.int32)


def robust(rays, scene, shift=1e-4, tol=1e-3):
    """bool [nray]: the reference gives the same geom and a distance within `tol` when the origin moves by +-shift along two
    directions perpendicular to the ray"""
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


# ------------------------------------------------------------------ independent method: march the membership test
def inside(gtype, X, size, hf=None):
    """bool [N]: points X (geom frame) inside the solid; a plane is the half space below it"""
    X = np.asarray(X, float).reshape(-1, 3)
    s = np.asarray(size, float)
    if gtype == PLANE: return X[:, 2] < 0
    if gtype == SPHERE: return np.linalg.norm(X, axis=1) < s[0]
    if gtype == ELLIPSOID: return np.linalg.norm(X / s, axis=1) < 1
    if gtype == CAPSULE:
        zc = np.clip(X[:, 2], -s[1], s[1])
        return np.linalg.norm(X - np.stack([0 * zc, 0 * zc, zc], axis=1), axis=1) < s[0]
    if gtype == CYLINDER: return (np.hypot(X[:, 0], X[:, 1]) < s[0]) & (np.abs(X[:, 2]) < s[1])
    if gtype == BOX: return (np.abs(X) < s).all(axis=1)
    if gtype == HFIELD:
        nrow, ncol, hs, data = hf
        inxy = (np.abs(X[:, 0]) < hs[0]) & (np.abs(X[:, 1]) < hs[1])
        return inxy & (X[:, 2] > -hs[3]) & (X[:, 2] < hfield_height(hf, np.clip(X[:, 0], -hs[0], hs[0]), np.clip(X[:, 1], -hs[1], hs[1])))
    raise ValueError(gtype)


def march(gtype, P, V, size, hf=None, length=8.0, step=1e-3, tol=1e-9):
    """distance (units of |V|) to the first change of inside() along each ray, -1 if there is none within `length` metres"""
    P = np.asarray(P, float).reshape(-1, 3); V = np.asarray(V, float).reshape(-1, 3)
    nv = np.linalg.norm(V, axis=1)
    U = V / nv[:, None]
    out = np.full(len(P), -1.0)
    ts = np.arange(0.0, length + step, step)
    for i in range(len(P)):
        ins = inside(gtype, P[i] + ts[:, None] * U[i], size, hf)
        k = np.nonzero(ins[1:] != ins[:-1])[0]
        if len(k) == 0:
            continue
        lo, hi, a = ts[k[0]], ts[k[0] + 1], ins[k[0]]
        while hi - lo > tol:
            mid = 0.5 * (lo + hi)
            if inside(gtype, P[i] + mid * U[i], size, hf)[0] == a: lo = mid
            else: hi = mid
        out[i] = 0.5 * (lo + hi) / nv[i]
    return out


# ------------------------------------------------------------------ scenes and ray sets (fixed seeds)
def quat2mat(q):
    w, x, y, z = q
    return np.array([w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),
                     2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z])


def random_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def rbound(gtype, s):
    return {SPHERE: s[0], CAPSULE: s[0] + s[1], ELLIPSOID: max(s), CYLINDER: float(np.hypot(s[0], s[1])), BOX: float(np.linalg.norm(s))}.get(gtype, 0.0)


PRIMITIVES = [(SPHERE, (0.22, 0, 0)), (CAPSULE, (0.12, 0.25, 0)), (ELLIPSOID, (0.3, 0.18, 0.12)), (CYLINDER, (0.18, 0.22, 0)),
              (BOX, (0.25, 0.15, 0.2))]


def primitives_spec(seed=11):
    """every primitive type once on the world body and once on a free body, at random poses over a bounded floor plane:
    list of dicts (type, size, pos, quat, free)"""
    rng = np.random.default_rng(seed)
    spec = [dict(type=PLANE, size=(3.0, 2.0, 0.05), pos=(0.0, 0.0, 0.0), quat=(1.0, 0, 0, 0), free=False)]
    cells = [(i, j) for i in range(-2, 3) for j in range(-1, 1)]
    for k, (t, s) in enumerate(PRIMITIVES + PRIMITIVES):
        cx, cy = cells[k]
        pos = (0.9 * cx + rng.uniform(-0.1, 0.1), 0.9 * cy + 0.45 + rng.uniform(-0.1, 0.1), rng.uniform(0.5, 1.5))
        spec.append(dict(type=t, size=s, pos=pos, quat=tuple(random_quat(rng)), free=k >= len(PRIMITIVES)))
    return spec


def scene_from_spec(spec, visible=None):
    n = len(spec)
    return dict(pos=np.array([g["pos"] for g in spec], float), mat=np.array([quat2mat(g["quat"]) for g in spec]),
                size=np.array([g["size"] for g in spec], float), type=np.array([g["type"] for g in spec]),
                visible=np.ones(n, bool) if visible is None else np.asarray(visible, bool), hfield={})


def scene_from_device(gpos, gmat, size, types, visible=None, hfield=None):
    """scene of one env from the device's own geom poses (mjh_get_geom_state)"""
    n = len(types)
    return dict(pos=np.asarray(gpos, float).reshape(n, 3), mat=np.asarray(gmat, float).reshape(n, 9), size=np.asarray(size, float).reshape(n, 3),
                type=np.asarray(types), visible=np.ones(n, bool) if visible is None else np.asarray(visible, bool), hfield=hfield or {})


def _is_inside_any(X, scene):
    bad = np.zeros(len(X), bool)
    for g in range(len(scene["type"])):
        t = int(scene["type"][g])
        if t == MESH or (t == HFIELD and g not in scene["hfield"]):
            continue
        R = scene["mat"][g].reshape(3, 3)
        bad |= inside(t, (X - scene["pos"][g]) @ R, scene["size"][g], scene["hfield"].get(g))
    return bad


def make_rays(seed, scene, nray, origin_lo, origin_hi, miss_share=0.2, miss_lift=1.0):
    """nray world-frame rays: origins uniform in the box [origin_lo, origin_hi] outside every geom, aimed at a point drawn inside
    half the bounding radius of a random geom (a plane / height field: a point of its footprint), directions of length 0.5 .. 2;
    a fixed share points away from the scene (outwards and, by miss_lift, up) and hits nothing"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(origin_lo, float), np.asarray(origin_hi, float)
    P = np.zeros((0, 3))
    while len(P) < nray:
        X = rng.uniform(lo, hi, size=(4 * nray, 3))
        P = np.vstack([P, X[~_is_inside_any(X, scene)]])
    P = P[:nray]
    ng = len(scene["type"])
    targets = [g for g in range(ng) if scene["visible"][g] and int(scene["type"][g]) != MESH]
    V = np.zeros((nray, 3))
    nmiss = int(round(miss_share * nray))
    for i in range(nray):
        if i >= nray - nmiss or not targets:
            d = P[i] - scene["pos"][targets].mean(axis=0) if targets else np.array([0, 0, 1.0])
            d[2] = abs(d[2]) + miss_lift
        else:
            g = targets[rng.integers(len(targets))]
            t = int(scene["type"][g]); R = scene["mat"][g].reshape(3, 3); s = scene["size"][g]
            if t == PLANE:
                ex = [s[0] if s[0] > 0 else 1.0, s[1] if s[1] > 0 else 1.0]
                loc = np.array([rng.uniform(-ex[0], ex[0]), rng.uniform(-ex[1], ex[1]), 0.0])
            elif t == HFIELD:
                hs = scene["hfield"][g][2]
                loc = np.array([rng.uniform(-hs[0], hs[0]), rng.uniform(-hs[1], hs[1]), rng.uniform(0, hs[2])])
            else:
                u = rng.normal(size=3); u /= np.linalg.norm(u)
                loc = u * 0.5 * rbound(t, s) * rng.uniform() ** (1 / 3)
            d = scene["pos"][g] + R @ loc - P[i]
        V[i] = d / np.linalg.norm(d) * rng.uniform(0.5, 2.0)
    return P, V


# the terrain of the height-field tests: 3 rows x 5 columns (unequal on purpose: a row / column swap changes every height)
HF_NROW, HF_NCOL = 3, 5
HF_SIZE = (1.0, 0.6, 0.4, 0.2)
HF_ELEV = np.array([[0.0, 0.3, 0.8, 0.5, 0.1], [0.2, 1.0, 0.4, 0.9, 0.3], [0.6, 0.1, 0.7, 0.2, 0.5]])     # already in [0, 1] with min 0, max 1
HF_POS = (0.3, -0.2, 0.25)
HF_QUAT = tuple(np.array([0.9, 0.1, -0.15, 0.4]) / np.linalg.norm([0.9, 0.1, -0.15, 0.4]))


def hfield_scene():
    hf = (HF_NROW, HF_NCOL, np.array(HF_SIZE), HF_ELEV)
    return dict(pos=np.array([HF_POS]), mat=np.array([quat2mat(HF_QUAT)]), size=np.zeros((1, 3)), type=np.array([HFIELD]),
                visible=np.ones(1, bool), hfield={0: hf})


def hfield_rays(scene, seed=5, nrand=100):
    """the directed cases of the height-field test (from above, through a wall, from below onto the base, along a cell diagonal,
    from inside the bounding box above the surface) in the geom's frame, moved to the world with its pose, plus random rays"""
    hf = scene["hfield"][0]
    sx, sy, sz, sb = hf[2]
    dx, dy = 2 * sx / (HF_NCOL - 1), 2 * sy / (HF_NROW - 1)
    loc = [
        ((0.13, 0.07, 2.0), (0, 0, -1.0)),                       # from above
        ((-0.61, 0.22, 1.5), (0.1, -0.05, -1.0)),
        ((-2.0, 0.11, -0.1), (1.0, 0.02, 0.0)),                  # through the x = -sx wall, below the terrain's edge
        ((0.37, 1.5, -0.05), (0.01, -1.0, 0.0)),                 # through the y = +sy wall
        ((-2.0, 0.11, 0.39), (1.0, 0.02, -0.05)),                # over the wall's top edge into the box, onto the terrain
        ((0.2, -0.1, -1.0), (0.05, 0.02, 1.0)),                  # from below onto the base
        ((-sx + 0.1 * dx, -sy + 0.1 * dy, 0.9), (dx, dy, -0.55)),  # along the cells' diagonal
        ((-sx + 0.1 * dx, -sy + 0.13 * dy, 0.9), (dx, dy, -0.55)),
        ((0.05, 0.02, 0.399), (0.7, 0.3, -0.2)),                 # origin inside the bounding box, above the surface
        ((-0.45, -0.25, 0.39), (-1.0, 0.1, 0.02)),               # ... leaving the box without touching anything
        ((0.1, 0.05, -0.1), (0.2, 0.1, 1.0)),                    # origin inside the solid: leaves through the top
        ((0.1, 0.05, -0.1), (1.0, 0.1, -0.02)),                  # ... through a wall
    ]
    R = scene["mat"][0].reshape(3, 3); t = scene["pos"][0]
    P = np.array([t + R @ np.array(p) for p, _ in loc]); V = np.array([R @ np.array(v) for _, v in loc])
    Pr, Vr = make_rays(seed, scene, nrand, (-2.5, -2.5, -1.5), (2.5, 2.5, 2.5))
    return np.vstack([P, Pr]), np.vstack([V, Vr])


# the terrains of the grid-line tests: cell indices up to 38 along y (A), along x (B), and a mid-sized grid (C)
TERRAINS = {"A": (40, 9, (1.5, 6.0, 1.0, 0.1), 61), "B": (9, 40, (6.0, 1.5, 1.0, 0.1), 62), "C": (17, 33, (4.0, 2.0, 0.6, 0.3), 63)}


def rolling(nrow, ncol, seed):
    """elevation [nrow, ncol] in [0, 1] with min 0 and max 1, exact in float32: rolling ground (two waves) under uniform noise"""
    rng = np.random.default_rng(seed)
    r, c = np.meshgrid(np.arange(nrow), np.arange(ncol), indexing="ij")
    e = np.sin(0.9 * r + rng.uniform(0, 6)) * np.cos(0.7 * c + rng.uniform(0, 6)) + 0.5 * np.sin(0.37 * (r + c) + rng.uniform(0, 6))
    e = e + rng.uniform(-0.4, 0.4, size=e.shape)
    e = (e - e.min()) / (e.max() - e.min())
    e = e.astype(np.float32).astype(float)
    e[e == e.max()] = 1.0; e[e == e.min()] = 0.0
    return e


def terrain(name):
    """hf tuple (nrow, ncol, size[4], elevation [nrow, ncol]) of terrain A, B or C (fixed seed)"""
    nrow, ncol, size, seed = TERRAINS[name]
    return nrow, ncol, np.array(size, float), rolling(nrow, ncol, seed)


def terrain_scene(hf):
    """the field alone, unrotated at the world origin: the world frame is the geom's"""
    return dict(pos=np.zeros((1, 3)), mat=np.eye(3).reshape(1, 9), size=np.zeros((1, 3)), type=np.array([HFIELD]), visible=np.ones(1, bool),
                hfield={0: hf})


def f32(*arrays):
    """rounded to float32 (kept as float64 arrays): the ray the device sees is the ray the reference sees"""
    out = tuple(np.asarray(a, float).astype(np.float32).astype(float) for a in arrays)
    return out if len(out) > 1 else out[0]


def grid_lines(hf):
    """x of every column line, y of every row line (fp64, as the reference places them)"""
    nrow, ncol, size, _ = hf
    return -size[0] + 2 * size[0] * np.arange(ncol) / (ncol - 1), -size[1] + 2 * size[1] * np.arange(nrow) / (nrow - 1)


def hfield_node_rays(hf):
    """straight down at every interior grid node: (P, V, (r, c) of each ray)"""
    nrow, ncol, size, _ = hf
    xs, ys = grid_lines(hf)
    rc = np.array([(r, c) for r in range(1, nrow - 1) for c in range(1, ncol - 1)])
    k = np.arange(len(rc))
    P = np.stack([xs[rc[:, 1]], ys[rc[:, 0]], size[2] + 0.25 + 0.05 * (k % 7)], axis=1)
    V = np.stack([0 * k, 0 * k, -0.5 - 0.25 * (k % 3)], axis=1).astype(float)
    return f32(P, V) + (rc,)


def hfield_line_rays(hf, axis, seed, nray=600):
    """rays in the vertical plane of an interior grid line: axis 1: a row line (vec.y == 0), axis 0: a column line (vec.x == 0); from
    beside and above the field onto a point of the line at terrain height"""
    nrow, ncol, size, _ = hf
    rng = np.random.default_rng(seed)
    lines = grid_lines(hf)[axis]
    o = 1 - axis
    P = np.zeros((nray, 3)); T = np.zeros((nray, 3))
    P[:, axis] = T[:, axis] = lines[rng.integers(1, len(lines) - 1, size=nray)]
    P[:, o] = rng.uniform(-size[o] - 1.0, size[o] + 1.0, size=nray); P[:, 2] = rng.uniform(size[2] + 0.2, size[2] + 1.5, size=nray)
    T[:, o] = rng.uniform(-size[o], size[o], size=nray); T[:, 2] = rng.uniform(0, size[2], size=nray)
    V = T - P
    V *= (rng.uniform(0.5, 2.0, size=nray) / np.linalg.norm(V, axis=1))[:, None]
    V[:, axis] = 0.0
    return f32(P, V)


def hfield_diagonal_rays(hf, seed, nray=400):
    """along the cells' diagonals through grid nodes: vec = +-(dx, dy, -z), the origin a whole number of cells up the diagonal from
    an interior node"""
    nrow, ncol, size, _ = hf
    rng = np.random.default_rng(seed)
    xs, ys = grid_lines(hf)
    dx, dy = xs[1] - xs[0], ys[1] - ys[0]
    r, c = rng.integers(1, nrow - 1, size=nray), rng.integers(1, ncol - 1, size=nray)
    k = rng.integers(1, 6, size=nray) * rng.choice([-1.0, 1.0], size=nray)       # cells back along the diagonal (either sense)
    zc = rng.uniform(0.15, 0.6, size=nray) * size[2]                             # descent per cell
    zn = rng.uniform(0.0, size[2], size=nray)                                    # the ray's height over the node
    P = np.stack([xs[c] - k * dx, ys[r] - k * dy, zn + np.abs(k) * zc], axis=1)
    V = np.stack([np.sign(k) * dx, np.sign(k) * dy, -zc], axis=1)
    return f32(P, V)


def hfield_grazing_rays(hf, seed, nray=400):
    """low rays started inside the field's box above the surface: a slope of at most 0.15 either way"""
    nrow, ncol, size, _ = hf
    rng = np.random.default_rng(seed)
    P = np.zeros((0, 3))
    while len(P) < nray:
        X = rng.uniform((-size[0], -size[1], 0.0), (size[0], size[1], size[2]), size=(4 * nray, 3))
        P = np.vstack([P, X[X[:, 2] > hfield_height(hf, X[:, 0], X[:, 1]) + 0.02]])
    P = P[:nray]
    a = rng.uniform(0, 2 * np.pi, size=nray)
    V = np.stack([np.cos(a), np.sin(a), rng.uniform(-0.15, 0.15, size=nray)], axis=1) * rng.uniform(0.5, 2.0, size=(nray, 1))
    return f32(P, V)


def hfield_random_rays(hf, seed, nray=400):
    size = hf[2]
    m = max(size[0], size[1]) + 1.0
    return f32(*make_rays(seed, terrain_scene(hf), nray, (-m, -m, -size[3] - 1.0), (m, m, size[2] + 2.0)))


def hfield_families(name, nrand=400):
    """every ray family of terrain `name` in the field's frame: list of (family name, (P, V)); diagonals on A and B only (on C one in
    eleven of them is non-robust, too close to the suites' cap of one in ten)"""
    hf = terrain(name)
    seed = TERRAINS[name][3] * 10
    out = [("nodes", hfield_node_rays(hf)[:2]), ("row planes", hfield_line_rays(hf, 1, seed + 1)), ("column planes", hfield_line_rays(hf, 0, seed + 2))]
    if name != "C":
        out.append(("diagonals", hfield_diagonal_rays(hf, seed + 3)))
    out += [("grazing", hfield_grazing_rays(hf, seed + 4)), ("random", hfield_random_rays(hf, seed + 5, nrand))]
    return out


# two height fields from two assets (C first: the second asset's data starts at 17 * 33), each tilted, side by side; a static box and
# a free sphere stand on the first
TWO_FIELDS_QUAT2 = tuple(np.array([0.93, -0.12, 0.1, 0.3]) / np.linalg.norm([0.93, -0.12, 0.1, 0.3]))


def two_fields_spec():
    """list of dicts as primitives_spec(), an hfield entry with its terrain's name under `terrain`"""
    posC, posA = np.array([0.0, 0.0, 0.3]), np.array([12.0, 0.5, 0.6])
    RC = quat2mat(HF_QUAT).reshape(3, 3)
    hfC = terrain("C")

    def on_c(x, y, lift):
        return tuple(posC + RC @ np.array([x, y, float(hfield_height(hfC, np.array([x]), np.array([y]))[0]) + lift]))
    return [dict(type=HFIELD, size=(0.0, 0.0, 0.0), pos=tuple(posC), quat=HF_QUAT, free=False, terrain="C"),
            dict(type=HFIELD, size=(0.0, 0.0, 0.0), pos=tuple(posA), quat=TWO_FIELDS_QUAT2, free=False, terrain="A"),
            dict(type=BOX, size=(0.3, 0.2, 0.25), pos=on_c(-1.3, 0.4, 0.45), quat=HF_QUAT, free=False),
            dict(type=SPHERE, size=(0.3, 0, 0), pos=on_c(1.6, -0.5, 0.4), quat=(1.0, 0, 0, 0), free=True)]


def two_fields_scene(spec=None):
    spec = spec or two_fields_spec()
    sc = scene_from_spec(spec)
    sc["hfield"] = {g: terrain(s["terrain"]) for g, s in enumerate(spec) if s["type"] == HFIELD}
    return sc


def two_fields_rays(scene, nray=300, seed=71):
    return f32(*make_rays(seed, scene, nray, (-6.0, -8.0, -3.0), (19.0, 8.0, 6.0)))


def level_spec():
    """an axis-aligned world: every solid type once, static and unrotated, round a scanner at the origin, on a bounded floor"""
    return [dict(type=PLANE, size=(4.0, 4.0, 0.05), pos=(0.0, 0.0, 0.0), quat=(1.0, 0, 0, 0), free=False),
            dict(type=BOX, size=(0.25, 0.15, 0.4), pos=(1.5, 0.0, 0.4), quat=(1.0, 0, 0, 0), free=False),
            dict(type=CYLINDER, size=(0.18, 0.4, 0), pos=(0.0, 1.6, 0.4), quat=(1.0, 0, 0, 0), free=False),
            dict(type=CAPSULE, size=(0.12, 0.3, 0), pos=(-1.5, 0.05, 0.45), quat=(1.0, 0, 0, 0), free=False),
            dict(type=ELLIPSOID, size=(0.3, 0.18, 0.25), pos=(0.2, -1.5, 0.3), quat=(1.0, 0, 0, 0), free=False),
            dict(type=SPHERE, size=(0.3, 0, 0), pos=(1.2, 1.2, 0.35), quat=(1.0, 0, 0, 0), free=False),
            dict(type=SPHERE, size=(0.05, 0, 0), pos=(40.0, 40.0, 50.0), quat=(1.0, 0, 0, 0), free=True)]      # (a model needs a moving body)


LEVEL_HEIGHTS = (0.2, 0.35, 0.5)


def level_rays():
    """a 360-beam horizontal fan (vec.z == 0) from the origin at three heights, then beams with two zero components: along +-x, +-y from
    the scanner, +-z from there, and along the cylinder's and the capsule's axis (on it, and beside it through the cap) from above and
    from below the floor"""
    a = np.deg2rad(np.arange(360) + 0.25)
    P = [np.stack([0 * a, 0 * a, 0 * a + h], axis=1) for h in LEVEL_HEIGHTS]
    V = [np.stack([np.cos(a), np.sin(a), 0 * a], axis=1) * (0.5 + 0.5 * k) for k in range(3)]
    ax = [((0, 0, 0.35), (1.0, 0, 0)), ((0, 0, 0.35), (-1.0, 0, 0)), ((0, 0, 0.35), (0, 2.0, 0)), ((0, 0, 0.35), (0, -0.5, 0)),
          ((0, 0, 0.35), (0, 0, -1.0)), ((0, 0, 0.35), (0, 0, 1.0)),
          ((0.0, 1.6, 2.0), (0, 0, -1.0)), ((0.05, 1.63, 2.0), (0, 0, -0.5)), ((0.05, 1.63, -1.0), (0, 0, 1.0)),       # the cylinder's axis
          ((-1.5, 0.05, 2.0), (0, 0, -1.0)), ((-1.45, 0.08, 2.0), (0, 0, -2.0)), ((-1.5, 0.05, -1.0), (0, 0, 1.0)),      # the capsule's
          ((1.2, 1.2, 3.0), (0, 0, -1.0)), ((0.2, -1.5, 3.0), (0, 0, -1.0)), ((1.5, 0.0, 3.0), (0, 0, -1.0)),
          ((3.0, 1.2, 0.35), (-1.0, 0, 0)), ((0.2, 3.0, 0.3), (0, -1.0, 0))]
    P.append(np.array([p for p, _ in ax], float)); V.append(np.array([v for _, v in ax], float))
    return f32(np.vstack(P), np.vstack(V))


def far_rays(scene, nray=130, seed=81):
    """the lines of primitive_rays, each origin moved back along its ray to 20 .. 30 m from the world's origin"""
    P, V = make_rays(seed, scene, nray, (-3.0, -2.0, 0.05), (3.0, 2.0, 3.0))
    rng = np.random.default_rng(seed + 1)
    U = V / np.linalg.norm(V, axis=1, keepdims=True)
    R = rng.uniform(20.0, 30.0, size=nray)
    pu = np.sum(P * U, axis=1)
    s = pu + np.sqrt(pu * pu - np.sum(P * P, axis=1) + R * R)
    return f32(P - s[:, None] * U, V)


def extreme_points(t, s):
    """the points of a geom farthest from its centre (geom frame): what a bounding sphere one ulp too tight would cut off"""
    if t == BOX:
        return np.array([[a * s[0], b * s[1], c * s[2]] for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)], float)
    if t == CYLINDER:
        return np.array([[s[0] * np.cos(a), s[0] * np.sin(a), z * s[1]] for z in (-1, 1) for a in np.arange(8) * np.pi / 4])
    if t == CAPSULE:
        return np.array([[0, 0, s[0] + s[1]], [0, 0, -s[0] - s[1]]], float)
    if t == ELLIPSOID:
        return np.array([[sg * s[k] if j == k else 0.0 for j in range(3)] for k in range(3) for sg in (-1, 1)])
    return np.zeros((0, 3))


def extreme_point_rays(scene, per_point=4, seed=91):
    """rays from random directions, 1 .. 2 m away, through 0.97 x every extreme point of every box, cylinder, capsule and ellipsoid:
    (P, V, target geom [nray], distance of the point along the ray in units of |vec| [nray]); origins above the floor, outside every geom"""
    rng = np.random.default_rng(seed)
    P, V, G, D = [], [], [], []
    for g in range(len(scene["type"])):
        t = int(scene["type"][g]); R = scene["mat"][g].reshape(3, 3)
        for q in extreme_points(t, scene["size"][g]):
            w = scene["pos"][g] + R @ (0.97 * q)
            k = 0
            while k < per_point:
                u = rng.normal(size=3); u /= np.linalg.norm(u)
                d = rng.uniform(1.0, 2.0)
                o = w - d * u
                if o[2] < 0.05 or _is_inside_any(o[None], scene)[0]:
                    continue
                ln = rng.uniform(0.5, 2.0)
                P.append(o); V.append(u * ln); G.append(g); D.append(d / ln); k += 1
    P, V = f32(np.array(P), np.array(V))
    return P, V, np.array(G), np.array(D)


FRAME_FAMILIES = ["random", "zero x", "zero y", "zero z", "along x", "along y", "along z"]


def frame_rays(t, s, family, dist, nray, seed):
    """rays in the frame of one primitive (a plane included), origins `dist` metres away, rounded to float32.  random: aimed at a point
    inside the geom (a plane: of its footprint); zero k: the same with component k of the origin moved to the target's, so that vec[k]
    is exactly 0; along k: parallel to axis k, the other two coordinates spread over 1.2 times the geom's extent (some rays pass by)"""
    rng = np.random.default_rng(seed)
    ext = np.array([s[0] if s[0] > 0 else 1.0, s[1] if s[1] > 0 else 1.0, 0.0]) if t == PLANE else \
        {SPHERE: np.full(3, s[0]), CAPSULE: np.array([s[0], s[0], s[0] + s[1]]), CYLINDER: np.array([s[0], s[0], s[1]])}.get(t, np.array(s, float))
    T = rng.uniform(-1, 1, size=(nray, 3)) * ext * 0.8
    u = rng.normal(size=(nray, 3))
    if t == PLANE:
        u[:, 2] = np.abs(u[:, 2]) + 0.05      # (from the front)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    kind, _, axis = family.partition(" ")
    k = "xyz".find(axis)
    if kind == "along":
        T = rng.uniform(-1, 1, size=(nray, 3)) * ext * 1.2
        u = np.zeros((nray, 3)); u[:, k] = rng.choice([-1.0, 1.0], size=nray)
    elif kind == "zero":
        u[:, k] = 0.0
        u /= np.linalg.norm(u, axis=1, keepdims=True)
    P, T = f32(T + dist * u, T)
    V = T - P
    V *= (rng.uniform(0.5, 2.0, size=nray) / np.linalg.norm(V, axis=1))[:, None]
    V = f32(V)
    if kind == "zero":
        V[:, k] = 0.0
    elif kind == "along":
        V[:, [j for j in range(3) if j != k]] = 0.0
    return P, V


def primitive_rays(scene, nray, seed=21):
    return make_rays(seed, scene, nray, (-3.0, -2.0, 0.05), (3.0, 2.0, 3.0))


def s24_rays(scene, nray, seed=31):
    """a scanner inside the pen: origins between the walls, below their tops, aimed at the boxes, the walls and the floor.
    (From outside, the pen is ambiguous: its four wall boxes overlap in the corners, where the outer faces and the tops of two walls
    are coplanar — a ray landing there has two geoms at exactly the same distance, and which of them an fp32 and an fp64 evaluation
    name is a coin toss no shift of the origin reveals.  From inside, two walls only share the corner's edge.)"""
    return make_rays(seed, scene, nray, (-0.15, -0.15, 0.05), (0.15, 0.15, 1.4), miss_lift=8.0)      # (steep enough to leave the pen without grazing a wall)


def many_spheres_spec(n=70, seed=41):
    """more static spheres than one staging pass of the kernel holds (64), on a grid over a floor"""
    rng = np.random.default_rng(seed)
    spec = [dict(type=PLANE, size=(0.0, 0.0, 0.05), pos=(0.0, 0.0, 0.0), quat=(1.0, 0, 0, 0), free=False)]
    for k in range(n):
        i, j = k % 10, k // 10
        spec.append(dict(type=SPHERE, size=(rng.uniform(0.08, 0.15), 0, 0), pos=(0.45 * (i - 4.5), 0.45 * (j - 3.0), rng.uniform(0.3, 1.2)),
                         quat=(1.0, 0, 0, 0), free=False))
    return spec


def pass_edge_spec(ngeom, seed=41):
    """many_spheres_spec() with exactly `ngeom` geoms, every one visible, the last sphere on a free body (a model needs a moving one):
    65 geoms leave the second staging pass of the kernels that trace per tile a single candidate, 130 reach a third pass.
    -> (spec, position of the last sphere)"""
    spec = many_spheres_spec(n=ngeom - 1, seed=seed)
    spec[-1] = dict(spec[-1], free=True)
    return spec, spec[-1]["pos"]


def many_spheres_rays(scene, nray=96, seed=43):
    return make_rays(seed, scene, nray, (-3.0, -2.5, 0.05), (3.0, 2.5, 3.0))


def mesh_model(lib):
    """a floor, two free bodies with a (box-shaped) mesh geom each and a static ball under the first: rays pass through the meshes"""
    import ctypes as C

    import mujoco_sim_amd as ms
    from helpers import D
    b = lib.mjh_builder_create()
    v = np.ascontiguousarray(np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * [0.2, 0.15, 0.1])
    mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
    assert mid >= 0
    lib.mjh_builder_add_geom(b, b"floor", 0, PLANE, D(0, 0, 0.05), None, None, None, -1, -1, -1, -1)
    for k in range(2):
        bd = lib.mjh_builder_add_body(b, b"m%d" % k, 0, D(0.9 * k, 0, 1.0), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        assert lib.mjh_builder_add_mesh_geom(b, b"mg%d" % k, bd, mid, None, None, None, -1, -1, -1, -1) >= 0
    lib.mjh_builder_add_geom(b, b"ball", 0, SPHERE, D(0.2, 0, 0), D(0, 0, 0.4), None, None, -1, -1, -1, -1)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    return m
