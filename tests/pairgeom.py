"""Independent geometry of the analytic narrow-phase pairs (numpy fp64 only) — a checker for plane-{sphere, capsule, cylinder,
ellipsoid, box, mesh}, sphere-sphere, sphere-capsule, capsule-capsule and sphere-box (oracle mjh_oracle.c, device dev_collide.h:
the same algorithms written twice, so their parity cannot see a mistake they share, nor one of the fp32 arithmetic alone).

Nothing here restates a routine under test.  What is checked are PROPERTIES of a reported contact list:

  * all pairs: the normal is unit, common to the list and points from geom 1 to geom 2; contacts exist iff the true signed distance
    is at most the margin; `pos - n dist/2` lies on geom 1's surface and `pos + n dist/2` on geom 2's (implicit function per type,
    `surface`); for a plane pair the first lies on the plane
  * sphere / capsule pairs: `dist` = the exact minimum of the axis distance over the parameter box (interior stationary point from
    the common perpendicular, the four edges, the corners: `seg_seg_dist`) minus the radii, and the axis points reconstructed from
    pos, n and dist lie on their segments.  Any minimiser passes: the closest pair of parallel axes is not unique
  * sphere-box: `dist` = signed distance of the centre to the box (negative inside) minus r; the sphere moved by dist n just touches
    the box (any of several tied faces passes)
  * plane pairs: n is the plane normal, the smallest dist is d0 - h(-n) with the textbook support function h of the type, every
    point lies on the geom at the height its dist states (cylinder: on a rim; box, mesh: a corner / vertex; capsule: on an end
    sphere — the higher end's lowest point is inside a tilted capsule by r (1 - cos tilt), not on it), the counts follow the
    documented rules (capsule: ends below the margin; box: corners below the margin and not above the centre, at most 4; cylinder
    1..4; ellipsoid, sphere 1; mesh at most 4, the deepest vertex among them)

A degenerate normal (concentric spheres, a sphere centre on a capsule axis, crossing axes, a sphere centre a hair outside a box) is
asked for its length and `dist` only.  `robust`: no include / exclude decision of the reference within 1e-4 of the margin; the
tests leave the others out (at most 2 % of a family).  `well_conditioned`: poses at which an fp32 and an fp64 evaluation of one
convention must agree point by point (used for the device - oracle comparison only).

The case generators (`cases`) build, per family, random poses (arbitrary rotations) and the directed edge poses of closed-form
contact code; the pair is placed at a target signed distance by bisection on `true_distance`.  Penetrations and gaps are
log-uniform in [2.5e-3, 0.3] x the smaller size and never below 1.2e-4 m: the lower end keeps the reference's own decisions out
of the 1e-4 m band (with sizes from 0.03 m, 1e-4 x size would put a third of every family inside it, against the 2 % cap)."""
import numpy as np

PLANE, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = 0, 2, 3, 4, 5, 6, 7
BAND = 1e-4
FAMILIES = ["plane_sphere", "plane_capsule", "plane_cylinder", "plane_ellipsoid", "plane_box", "plane_mesh",
            "sphere_sphere", "sphere_capsule", "capsule_capsule", "sphere_box"]
TYPES = dict(plane=PLANE, sphere=SPHERE, capsule=CAPSULE, ellipsoid=ELLIPSOID, cylinder=CYLINDER, box=BOX, mesh=MESH)
SIGNS = np.array([[a, b, c] for c in (-1, 1) for b in (-1, 1) for a in (-1, 1)], dtype=np.float64)
norm = np.linalg.norm


# ---- quaternions (w, x, y, z); R's columns are the geom's axes
def quat_mul(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def quat_mat(q):
    w, x, y, z = q
    return np.array([[w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y)], [2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x)],
                     [2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z]])


def rot_quat(axis, ang):
    a = np.asarray(axis, float); a = a / norm(a)
    return np.r_[np.cos(ang / 2), np.sin(ang / 2) * a]


def rand_quat(rng):
    q = rng.normal(size=4)
    return q / norm(q)


def geom(t, p, q, s):
    return (t, np.asarray(p, float), quat_mat(np.asarray(q, float)), np.asarray(s, float))


# ---- surfaces: an implicit function per type, zero on the surface, in metres (exact distance except for the ellipsoid: first order)
_hulls = {}


def _hull(V):
    key = V.tobytes()
    if key not in _hulls:
        from scipy.spatial import ConvexHull
        _hulls[key] = ConvexHull(V).equations
    return _hulls[key]


def surface(g, x):
    t, p, R, s = g
    l = R.T @ (np.asarray(x, float) - p)
    if t == PLANE:
        return l[2]
    if t == SPHERE:
        return norm(l) - s[0]
    if t == CAPSULE:
        return np.hypot(np.hypot(l[0], l[1]), max(abs(l[2]) - s[1], 0.0)) - s[0]
    if t == ELLIPSOID:
        k = norm(l / s)
        return -s.min() if k == 0 else (k - 1) * k / norm(l / (s * s))
    if t == CYLINDER:
        dr, dz = np.hypot(l[0], l[1]) - s[0], abs(l[2]) - s[1]
        return np.hypot(max(dr, 0.0), max(dz, 0.0)) + min(max(dr, dz), 0.0)
    if t == BOX:
        q = np.abs(l) - s[:3]
        return norm(np.maximum(q, 0)) + min(q.max(), 0.0)
    if t == MESH:
        E = _hull(s)
        return float((E[:, :3] @ l + E[:, 3]).max())
    raise ValueError(t)


def support(g, d):
    """textbook support function h(d) = max over the geom of d . (x - centre), d unit"""
    t, p, R, s = g
    if t == SPHERE:
        return s[0]
    if t == CAPSULE:
        return s[0] + s[1] * abs(R[:, 2] @ d)
    if t == CYLINDER:      # (the sine from the cross product: 1 - cos^2 of axes that are unit to 1e-7 only is off by 2e-7, a tilt of 4e-4)
        a = R[:, 2] / norm(R[:, 2])
        return s[1] * abs(a @ d) + s[0] * norm(_cross(a, d))
    if t == ELLIPSOID:
        return np.sqrt(np.sum((s[:3] * (R.T @ d)) ** 2))
    if t == BOX:
        return np.sum(s[:3] * np.abs(R.T @ d))
    if t == MESH:
        return float((s @ (R.T @ d)).max())
    raise ValueError(t)


# ---- segments: a sphere is a segment of half length 0
def _seg(g):
    return g[1], g[2][:, 2], (g[3][1] if g[0] == CAPSULE else 0.0), g[3][0]


def _cross(a, b):
    return np.array([a[1]*b[2] - a[2]*b[1], a[2]*b[0] - a[0]*b[2], a[0]*b[1] - a[1]*b[0]])


def seg_point_dist(c, a, h, x):
    """exact minimum over [-h, h]: the interior stationary point (if inside) and the two ends"""
    t0 = a @ (x - c)
    return min(norm(x - (c + t * a)) for t in ([-h, h] + ([t0] if -h < t0 < h else [])))


def seg_seg_dist(c1, a1, h1, c2, a2, h2):
    """exact minimum of |c1 + x1 a1 - c2 - x2 a2| over [-h1, h1] x [-h2, h2]: a convex quadratic over a box has its minimum at the
    interior stationary point (the common perpendicular) if that lies inside, else on an edge (1-D minimum) or at a corner"""
    best = min(norm(c1 + s * a1 - c2 - t * a2) for s in (-h1, h1) for t in (-h2, h2))
    for s in (-h1, h1):
        best = min(best, seg_point_dist(c2, a2, h2, c1 + s * a1))
    for t in (-h2, h2):
        best = min(best, seg_point_dist(c1, a1, h1, c2 + t * a2))
    n = _cross(a1, a2)
    if h1 > 0 and h2 > 0 and n @ n > 1e-28:
        # c1 + y0 a1 + y2 n = c2 + y1 a2 (Cramer's rule; the system's determinant is -|n|^2)
        b = c2 - c1
        y0, y1 = b @ _cross(a2, n) / (n @ n), b @ _cross(a1, n) / (n @ n)
        if abs(y0) <= h1 and abs(y1) <= h2:
            best = min(best, norm(c1 + y0 * a1 - c2 - y1 * a2))
    return best


def axis_distance(g1, g2):
    c1, a1, h1, _ = _seg(g1); c2, a2, h2, _ = _seg(g2)
    return seg_seg_dist(c1, a1, h1, c2, a2, h2)


def true_distance(g1, g2):
    t1, t2 = g1[0], g2[0]
    if t1 == PLANE:
        n = g1[2][:, 2]
        return n @ (g2[1] - g1[1]) - support(g2, -n)
    if t2 == BOX:
        return surface(g2, g1[1]) - g1[3][0]
    return axis_distance(g1, g2) - g1[3][0] - g2[3][0]


def _plane_heights(g1, g2):
    """heights above the plane of the candidate points whose inclusion the convention decides (every one, per type)"""
    t, c, R, s = g2
    n, d0 = g1[2][:, 2], g1[2][:, 2] @ (g2[1] - g1[1])
    if t == CAPSULE:
        return np.array([d0 + e * s[1] * (R[:, 2] @ n) - s[0] for e in (1, -1)])
    if t == BOX:
        return d0 + (SIGNS * s[:3]) @ (R.T @ n)
    if t == MESH:
        return d0 + s @ (R.T @ n)
    if t == CYLINDER:      # deepest rim point, the same rim direction on the far cap, the near cap's rim at +-120 degrees
        a = R[:, 2] / norm(R[:, 2]); ca = abs(a @ n) / norm(n); sa = norm(_cross(a, n)) / norm(n)
        return np.array([d0 - s[1] * ca - s[0] * sa, d0 + s[1] * ca - s[0] * sa, d0 - s[1] * ca + 0.5 * s[0] * sa])
    return np.array([true_distance(g1, g2)])


def robust(g1, g2, margin, band=BAND, D=None):
    """no include / exclude decision of the reference within `band` of its threshold (D: the true distance, if already known)"""
    if abs((true_distance(g1, g2) if D is None else D) - margin) < band:
        return False
    if g1[0] == PLANE:
        hgt = _plane_heights(g1, g2)
        if (np.abs(hgt - margin) < band).any():
            return False
        if g2[0] == BOX:       # "not above the centre"
            ld = (SIGNS * g2[3][:3]) @ (g2[2].T @ g1[2][:, 2])
            if ((np.abs(ld) < band) & (hgt <= margin + band)).any():
                return False
    return True


def degenerate(g1, g2, eps, D=None):
    """the normal is not determined (to rounding of size eps / distance): only its length and `dist` are asked for"""
    if g1[0] == PLANE:
        return False
    D = true_distance(g1, g2) if D is None else D
    return 0 < D + g1[3][0] < eps if g2[0] == BOX else D + g1[3][0] + g2[3][0] < eps


def axis_angle(g1, g2):
    return float(np.arcsin(min(1.0, norm(np.cross(g1[2][:, 2], g2[2][:, 2])))))


def well_conditioned(g1, g2, margin=0.0):
    """poses at which two evaluations of one convention in different precision must report the same points in the same order"""
    if not robust(g1, g2, margin) or degenerate(g1, g2, 1e-3):
        return False
    t1, t2 = g1[0], g2[0]
    if t1 == CAPSULE and t2 == CAPSULE:
        # the stationary point's parameters carry the operands' rounding (6e-8 at 0.5 m) divided by angle^2: 6e-4 m at 1e-2 rad,
        # 6e-6 m at 0.1 rad.  Points compare to 2e-5 from 0.1 rad on, and from 1e-2 rad where the stationary point lies outside
        # the parameter box by more than that error (the minimum is then on an edge, which needs no such division)
        ang = axis_angle(g1, g2)
        if ang <= 1e-2:
            return False
        c1, a1, h1, _ = _seg(g1); c2, a2, h2, _ = _seg(g2)
        n = _cross(a1, a2); b = c2 - c1
        y0, y1 = b @ _cross(a2, n) / (n @ n), b @ _cross(a1, n) / (n @ n)
        return ang > 0.1 or (ang > 1e-2 and (abs(y0) > h1 + 1e-2 or abs(y1) > h2 + 1e-2))
    if t2 == BOX and t1 == SPHERE:
        q = np.sort(g2[3][:3] - np.abs(g2[2].T @ (g1[1] - g2[1])))
        return q[0] < 0 or q[1] - q[0] > 1e-3         # inside: the nearest face is not tied
    if t1 == PLANE and t2 == CYLINDER:
        c = abs(g2[2][:, 2] @ g1[2][:, 2])
        return 1e-2 < c < np.cos(1e-2)                 # neither standing (rim direction) nor lying (which cap is the near one)
    if t1 == PLANE and t2 == MESH:
        h = np.sort(_plane_heights(g1, g2))
        return h[1] - h[0] > 1e-3
    return True


# ---- the checker
def _near_any(x, P, tol):
    d = norm(P - x, axis=1)
    i = int(np.argmin(d))
    return i if d[i] <= tol else -1


def _check_plane(g1, g2, margin, dist, pos, n, tol, ctol, bad):
    t, c, R, s = g2
    pn, pp = g1[2][:, 2], g1[1]
    k = len(dist)
    if norm(n - pn) > 10 * tol:
        bad.append(f"normal {n} is not the plane's {pn}")
    dmin = pn @ (c - pp) - support(g2, -pn)
    if abs(dist.min() - dmin) > tol:
        bad.append(f"smallest dist {dist.min():.9e}, support function gives {dmin:.9e}")
    X = pos + 0.5 * dist[:, None] * n
    Y = pos - 0.5 * dist[:, None] * n
    for q in range(k):
        if abs(pn @ (Y[q] - pp)) > tol:
            bad.append(f"point {q}: pos - n dist/2 is {pn @ (Y[q] - pp):.3e} off the plane")
        # (a capsule's contacts are the lowest points of its two END SPHERES, MuJoCo's convention: the higher end's lies inside the
        #  capsule by r (1 - cos tilt); the deepest one is on the capsule itself and is asked for that)
        f = surface(g2, X[q]) if t != CAPSULE or dist[q] == dist.min() else min((abs(norm(X[q] - c - e * s[1] * R[:, 2]) - s[0]) for e in (1, -1)))
        if abs(f) > tol:
            bad.append(f"point {q}: pos + n dist/2 is {f:.3e} off the geom's surface")
        for r in range(q):
            if norm(X[q] - X[r]) <= ctol:
                bad.append(f"points {r} and {q} coincide")
    hgt = _plane_heights(g1, g2)
    if t in (SPHERE, ELLIPSOID) and k != 1:
        bad.append(f"{k} contacts, the pair has one")
    elif t == CAPSULE:
        ends = np.array([c + e * s[1] * R[:, 2] - s[0] * pn for e in (1, -1)])
        hit = [_near_any(X[q], ends, tol) for q in range(k)]
        if -1 in hit:
            bad.append("a point is not the lowest point of an end sphere")
        for e in range(2):
            if hgt[e] < margin - ctol and e not in hit:
                bad.append(f"end {e} at {hgt[e]:.3e} below the margin has no contact")
            if hgt[e] > margin + ctol and e in hit:
                bad.append(f"end {e} at {hgt[e]:.3e} above the margin has a contact")
    elif t == BOX:
        corners = c + (SIGNS * s[:3]) @ R.T
        ld = hgt - pn @ (c - pp)
        hit = [_near_any(X[q], corners, tol) for q in range(k)]
        if -1 in hit:
            bad.append("a point is not a corner")
        for i in hit:
            if i >= 0 and (hgt[i] > margin + ctol or ld[i] > ctol):
                bad.append(f"corner {i} reported: height {hgt[i]:.3e}, {ld[i]:.3e} above the centre")
        must = [i for i in range(8) if hgt[i] < margin - ctol and ld[i] < -ctol]
        if k > 4:
            bad.append(f"{k} contacts, at most 4")
        if k < min(4, len(must)) or (k < 4 and any(i not in hit for i in must)):
            bad.append(f"{k} contacts, {len(must)} corners are below the margin and the centre")
    elif t == CYLINDER:
        if not 1 <= k <= 4:
            bad.append(f"{k} contacts, 1 to 4")
        for q in range(k):
            l = R.T @ (X[q] - c)
            if abs(abs(l[2]) - s[1]) > tol or abs(np.hypot(l[0], l[1]) - s[0]) > tol:
                bad.append(f"point {q} is not on a rim")
    elif t == MESH:
        V = c + s @ R.T
        hit = [_near_any(X[q], V, tol) for q in range(k)]
        if -1 in hit:
            bad.append("a point is not a vertex")
        if k > 4:
            bad.append(f"{k} contacts, at most 4")
        for i in hit:
            if i >= 0 and hgt[i] > margin + ctol:
                bad.append(f"vertex {i} at {hgt[i]:.3e} above the margin reported")


def _check_round(g1, g2, margin, dist, pos, n, tol, bad, D):
    if len(dist) != 1:
        bad.append(f"{len(dist)} contacts, the pair has one")
        return
    d, x = float(dist[0]), pos[0]
    r1 = g1[3][0]
    if abs(d - D) > tol:
        bad.append(f"dist {d:.9e}, true distance {D:.9e} ({d - D:+.3e})")
    if degenerate(g1, g2, 10 * tol, D):
        return
    for g, sg, name in ((g1, -1.0, "geom 1"), (g2, 1.0, "geom 2")):
        f = surface(g, x + sg * 0.5 * d * n)
        if abs(f) > tol:
            bad.append(f"pos {'-' if sg < 0 else '+'} n dist/2 is {f:.3e} off {name}'s surface")
    if g2[0] == BOX:
        f = surface(g2, g1[1] + d * n) - r1
        if abs(f) > tol:
            bad.append(f"the sphere moved by dist n is {f:.3e} from just touching the box")
        return
    for g, sg, name in ((g1, -1.0, "1"), (g2, 1.0, "2")):
        c, a, h, r = _seg(g)
        f = seg_point_dist(c, a, h, x + sg * (0.5 * d + r) * n)
        if f > tol:
            bad.append(f"the reconstructed axis point of geom {name} is {f:.3e} off its segment")


def check_contacts(geom1, geom2, margin, dist, pos, normal, tol=1e-9, count_tol=None, D=None):
    """Returns a list of violation strings (empty: the contact list passes).  geom = (type, p[3], R[3,3] columns = axes, size[3] — for
    a mesh its vertices [nv, 3] in the geom frame); dist[k], pos[k, 3], normal[3] or [k, 3] as reported (k may be 0).  `tol`:
    absolute length tolerance; `count_tol` (default 10 tol): a decision closer than this to its threshold may go either way; `D`:
    true_distance(geom1, geom2), if the caller has it already."""
    dist = np.atleast_1d(np.asarray(dist, float)); pos = np.asarray(pos, float).reshape(-1, 3)
    N = np.asarray(normal, float).reshape(-1, 3)
    ctol = 10 * tol if count_tol is None else count_tol
    k = len(dist)
    D = true_distance(geom1, geom2) if D is None else D
    bad = []
    if k == 0:
        if D < margin - tol:
            bad.append(f"no contact although the true distance is {D:.6e} <= margin {margin}")
        return bad
    if D > margin + tol:
        return [f"{k} contacts although the true distance is {D:.6e} > margin {margin}"]
    n = N[0]
    if len(N) not in (1, k) or np.abs(N - n).max() > 10 * tol:
        bad.append("the contacts of the pair do not share one normal")
    if abs(norm(n) - 1) > 10 * tol:
        bad.append(f"|n| = {norm(n)}")
    if (dist > margin + tol).any():
        bad.append(f"dist {dist.max():.3e} beyond the margin")
    if geom1[0] == PLANE:
        _check_plane(geom1, geom2, margin, dist, pos, n, tol, ctol, bad)
    else:
        _check_round(geom1, geom2, margin, dist, pos, n, tol, bad, D)
    return bad


# ---- case generators
def _logu(rng, lo, hi):
    return float(np.exp(rng.uniform(np.log(lo), np.log(hi))))


def _target(rng, size, p_sep=0.2):
    """signed target distance: a penetration (or, for a share p_sep, a gap) log-uniform in [2.5e-3, 0.3] x size, at least 1.2e-4 m"""
    d = _logu(rng, max(2.5e-3 * size, 1.2 * BAND), 0.3 * size)
    return d if rng.random() < p_sep else -d


def _place(make, fixed, target, thi, first):
    """t in [0, thi] with true_distance = target to 1e-7 (regula falsi, Illinois variant; the distance grows with t on the bracket)"""
    f = (lambda t: true_distance(make(t), fixed) - target) if first else (lambda t: true_distance(fixed, make(t)) - target)
    lo, hi = 0.0, thi
    flo, fhi = f(lo), f(hi)
    if flo > 0 or fhi < 0:
        return hi if fhi < 0 else lo
    for _ in range(30):
        mid = hi - fhi * (hi - lo) / (fhi - flo)
        fm = f(mid)
        if abs(fm) < 1e-7:
            return mid
        if fm < 0:
            lo, flo, fhi = mid, fm, (fhi if fhi * flo < 0 and _ == 0 else 0.5 * fhi)
        else:
            hi, fhi, flo = mid, fm, 0.5 * flo
    return mid


def _perp(rng, a):
    u = np.cross(a, rng.normal(size=3))
    return u / norm(u)


def _sizes(rng, t, i):
    if t == SPHERE:
        return np.array([rng.uniform(0.03, 0.1), 0, 0])
    if t == CAPSULE:
        return np.array([rng.uniform(0.03, 0.08), rng.uniform(0.03, 0.2), 0])
    if t == CYLINDER:
        return np.array([rng.uniform(0.03, 0.08), rng.uniform(0.03, 0.15), 0])
    if t == BOX:
        return rng.uniform(0.04, 0.125, 3)
    if t == ELLIPSOID:      # aspect ratios up to 10 : 1
        return rng.uniform(0.08, 0.12) * np.array([1.0, _logu(rng, 0.1, 1), _logu(rng, 0.1, 1)])[rng.permutation(3)]
    raise ValueError(t)


HALF = np.sqrt(0.5)
FACE_QUATS = [np.array([1.0, 0, 0, 0]), np.array([HALF, HALF, 0, 0]), np.array([HALF, 0, HALF, 0])]


def _plane_case(rng, i, name, plane_q, plane_p, mesh):
    t2 = TYPES[name]
    g1 = geom(PLANE, plane_p, plane_q, [0, 0, 0])
    s = mesh if t2 == MESH else _sizes(rng, t2, i)
    spin = quat_mul(plane_q, rot_quat([0, 0, 1], rng.uniform(0, 2 * np.pi)))
    mode = i % 8
    tag = "random"
    q = rand_quat(rng)
    if t2 in (CAPSULE, CYLINDER) and mode < 6:
        base = 0.0 if mode < 3 else np.pi / 2                       # standing / lying
        if mode % 3 == 0:
            ang, tag = 0.0, ("standing" if mode < 3 else "lying")
        else:
            ang = _logu(rng, 1e-7, 1e-1) * rng.choice([-1, 1]); tag = ("near-standing" if mode < 3 else "near-lying")
        flip = np.pi if (mode < 3 and rng.random() < 0.5) else 0.0
        q = quat_mul(spin, rot_quat([1, 0, 0], base + ang + flip))
    elif t2 == BOX and mode < 6:
        face = FACE_QUATS[rng.integers(3)]
        if mode in (0, 1):
            q, tag = quat_mul(spin, face), "flat"
        elif mode in (2, 3):
            q, tag = quat_mul(quat_mul(spin, face), rot_quat(rng.normal(size=3), 1e-6)), "flat tilted 1e-6"
        elif mode == 4:
            q, tag = quat_mul(quat_mul(spin, face), rot_quat([1, 0, 0], rng.uniform(0.2, np.pi / 2 - 0.2))), "edge"
        else:               # a body diagonal along the normal: on a corner
            d = s[:3] / norm(s[:3]); ax = np.cross(d, [0, 0, 1.0]); an = np.arccos(d[2])
            q, tag = quat_mul(spin, rot_quat(ax, an)), "corner"
    elif t2 == ELLIPSOID and mode < 4:
        q, tag = quat_mul(spin, FACE_QUATS[rng.integers(3)]), "axis-aligned"
    elif t2 == MESH and mode < 3:      # resting on a facet: several vertices at one height
        E = _hull(mesh); fn = E[rng.integers(len(E)), :3]
        ax = np.cross(fn, [0, 0, -1.0]); an = np.arccos(np.clip(-fn[2], -1, 1))
        q, tag = quat_mul(spin, rot_quat(ax if norm(ax) > 1e-12 else [1, 0, 0], an)), "facet"
    n = g1[2][:, 2]
    size = float(np.min(s[:2 if t2 in (CAPSULE, CYLINDER) else 3])) if t2 not in (SPHERE, MESH) else (s[0] if t2 == SPHERE else 0.05)
    g2 = geom(t2, [0, 0, 0], q, s)
    lat = g1[2] @ np.r_[rng.uniform(-0.3, 0.3, 2), 0]
    c = plane_p + lat + n * (_target(rng, size) + support(g2, -n))
    return dict(g1=g1, g2=(t2, c, g2[2], g2[3]), q1=plane_q, q2=q, tag=tag)


def _round_case(rng, i, family):
    c1 = rng.uniform(-0.4, 0.4, 3)
    mode = i % 8
    far = 1.0
    if family == "sphere_sphere":
        s1, s2 = _sizes(rng, SPHERE, i), _sizes(rng, SPHERE, i)
        q1 = q2 = np.array([1.0, 0, 0, 0])
        d = rng.normal(size=3); d /= norm(d)
        if mode == 0:
            return dict(g1=geom(SPHERE, c1, q1, s1), g2=geom(SPHERE, c1, q2, s2), q1=q1, q2=q2, tag="concentric")
        size = min(s1[0], s2[0])
        tgt = _target(rng, size) if mode > 2 else rng.choice([-1, 1]) * _logu(rng, 1.2e-4, 1e-3)      # grazing: just outside the band
        return dict(g1=geom(SPHERE, c1, q1, s1), g2=geom(SPHERE, c1 + d * (s1[0] + s2[0] + tgt), q2, s2), q1=q1, q2=q2,
                    tag="random" if mode > 2 else "grazing")
    if family == "sphere_capsule":
        s1, s2 = _sizes(rng, SPHERE, i), _sizes(rng, CAPSULE, i)
        q1, q2 = np.array([1.0, 0, 0, 0]), rand_quat(rng)
        g2 = geom(CAPSULE, c1, q2, s2); a = g2[2][:, 2]; u = _perp(rng, a)
        tgt = _target(rng, min(s1[0], s2[0]))
        if mode == 0:      # centre on the axis, inside the segment
            return dict(g1=geom(SPHERE, c1 + a * rng.uniform(-1, 1) * s2[1], q1, s1), g2=g2, q1=q1, q2=q2, tag="on the axis")
        if mode == 1:      # centre on the axis, beyond a cap
            o, d, tag = np.zeros(3), a * rng.choice([-1, 1]), "on the axis beyond a cap"
        elif mode in (2, 3):  # beyond a cap, off the axis
            o, d, tag = u * rng.uniform(0, 0.5) * s2[0], a * rng.choice([-1, 1]), "beyond a cap"
        elif mode in (4, 5):
            o, d, tag = a * rng.uniform(-1, 1) * s2[1], u, "beside the shaft"
        else:
            o, d, tag = np.zeros(3), rand_quat(rng)[:3], "random"; d = d / norm(d)
        t = _place(lambda t: geom(SPHERE, c1 + o + t * d, q1, s1), g2, tgt, far, True)
        return dict(g1=geom(SPHERE, c1 + o + t * d, q1, s1), g2=g2, q1=q1, q2=q2, tag=tag)
    if family == "sphere_box":
        s1, s2 = _sizes(rng, SPHERE, i), _sizes(rng, BOX, i)
        if mode == 7:
            s1 = np.array([rng.uniform(0.004, 0.008), 0, 0])        # a sphere much smaller than the box
        q1, q2 = np.array([1.0, 0, 0, 0]), rand_quat(rng)
        g2 = geom(BOX, c1, q2, s2); R = g2[2]; s = s2[:3]
        k = int(rng.integers(3)); j = (k + 1 + int(rng.integers(2))) % 3; sg = rng.choice([-1.0, 1.0], 3)
        loc = None
        m16 = i % 16
        if m16 == 0:
            loc, tag = np.zeros(3), "box centre"
        elif m16 == 8:      # centre on a face plane, over the face
            loc = rng.uniform(-0.8, 0.8, 3) * s; loc[k] = sg[k] * s[k]; tag = "on a face"
        elif mode == 1:     # inside, near one face
            loc = rng.uniform(-0.3, 0.3, 3) * s; loc[k] = sg[k] * (s[k] - _logu(rng, 2e-4, 0.3) * s.min()); tag = "inside near a face"
        elif mode == 2:     # inside, near two faces (every fourth: exactly tied)
            loc = rng.uniform(-0.3, 0.3, 3) * s; dk = _logu(rng, 2e-4, 0.2) * s.min()
            dj = dk if (i // 8) % 4 == 0 else dk * rng.uniform(1.0, 1.5)
            loc[k] = sg[k] * (s[k] - dk); loc[j] = sg[j] * (s[j] - dj); tag = "inside near two faces"
        if loc is not None:
            return dict(g1=geom(SPHERE, c1 + R @ loc, q1, s1), g2=g2, q1=q1, q2=q2, tag=tag)
        tgt = _target(rng, min(s1[0], s.min()))
        if mode in (0, 3):  # facing a face
            o = rng.uniform(-0.9, 0.9, 3) * s; o[k] = 0; d = np.zeros(3); d[k] = sg[k]; tag = "face"
        elif mode == 4:     # facing an edge: from a point of the edge, outwards between the two faces
            o = sg * s; l = 3 - k - j; o[l] = rng.uniform(-0.9, 0.9) * s[l]; o = o * 0.999
            w = rng.uniform(0.1, 0.9); d = np.zeros(3); d[k] = sg[k] * w; d[j] = sg[j] * (1 - w); tag = "edge"
        elif mode == 5:     # facing a corner
            o = sg * s * 0.999; d = sg * rng.uniform(0.1, 1, 3); tag = "corner"
        else:
            o, d, tag = np.zeros(3), rng.normal(size=3), "random"
        d = d / norm(d)
        t = _place(lambda t: geom(SPHERE, c1 + R @ (o + t * d), q1, s1), g2, tgt, far, True)
        return dict(g1=geom(SPHERE, c1 + R @ (o + t * d), q1, s1), g2=g2, q1=q1, q2=q2, tag=tag)
    # capsule_capsule: half of the cases closer than 1e-3 rad
    s1, s2 = _sizes(rng, CAPSULE, i), _sizes(rng, CAPSULE, i)
    if (i // 8) % 3 == 0:
        s2[1] = s1[1]                                                   # equal lengths
    q1 = rand_quat(rng)
    g1 = geom(CAPSULE, c1, q1, s1); a1 = g1[2][:, 2]; u = _perp(rng, a1)
    tgt = _target(rng, min(s1[0], s2[0]))
    if mode < 5:
        if mode == 0:
            q2, tag = q1.copy(), "parallel"
        elif mode == 1:
            q2, tag = quat_mul(q1, rot_quat([1, 0, 0], np.pi)), "antiparallel"
        else:
            ang = _logu(rng, 1e-7, 1e-3) if mode < 4 else _logu(rng, 1e-3, 1e-1)
            q2, tag = quat_mul(q1, rot_quat(np.r_[rng.normal(size=2), 0], ang)), "near-parallel"
        sub = (i // 8) % 4
        if sub == 0:        # overlapping, side by side
            o, d = a1 * rng.uniform(-0.5, 0.5) * abs(s1[1] - s2[1] + 1e-3), u; tag += " overlapping"
        elif sub == 1:      # partly overlapping
            o, d = a1 * rng.choice([-1, 1]) * rng.uniform(0.5, 0.98) * (s1[1] + s2[1]), u; tag += " partly overlapping"
        elif sub == 2:      # collinear, end to end
            o, d = np.zeros(3), a1 * rng.choice([-1, 1]); tag += " end to end"
        else:               # beyond the end, off the axis
            o, d = u * rng.uniform(0.1, 0.9) * (s1[0] + s2[0]), a1 * rng.choice([-1, 1]); tag += " beyond the end"
    elif mode == 5:
        w = np.cross(a1, u)
        q2 = quat_mul(q1, rot_quat([1, 0, 0], np.pi / 2))
        a2 = quat_mat(q2)[:, 2]
        if (i // 8) % 2 == 0:   # T: an end of capsule 2 against the shaft of capsule 1
            o, d, tag = a1 * rng.uniform(-0.8, 0.8) * s1[1], a2 * rng.choice([-1, 1]), "T"
        elif (i // 8) % 4 == 1:  # crossing axes that meet
            g2 = geom(CAPSULE, c1 + a1 * rng.uniform(-0.8, 0.8) * s1[1] + a2 * rng.uniform(-0.8, 0.8) * s2[1], q2, s2)
            return dict(g1=g1, g2=g2, q1=q1, q2=q2, tag="crossing, axes meet")
        else:
            w = np.cross(a1, a2)
            o, d, tag = a1 * rng.uniform(-0.8, 0.8) * s1[1] + a2 * rng.uniform(-0.8, 0.8) * s2[1], w * rng.choice([-1, 1]), "crossing"
    else:
        q2 = rand_quat(rng)
        o, d, tag = np.zeros(3), rng.normal(size=3), "random"
    d = d / norm(d)
    t = _place(lambda t: geom(CAPSULE, c1 + o + t * d, q2, s2), g1, tgt, far, False)
    return dict(g1=g1, g2=geom(CAPSULE, c1 + o + t * d, q2, s2), q1=q1, q2=q2, tag=tag)


def cases(family, n, seed, plane=None, mesh=None):
    """n cases of a family: dicts g1, g2 (geoms), q1, q2 (their quaternions), tag.  plane = (quat, pos) of the static plane and
    mesh = vertices in the geom frame, for the plane families"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        if family.startswith("plane_"):
            out.append(_plane_case(rng, i, family[6:], np.asarray(plane[0], float), np.asarray(plane[1], float), mesh))
        else:
            out.append(_round_case(rng, i, family))
    return out
