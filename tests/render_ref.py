"""fp64 numpy reference for RGB-D images (mjh_render): beside ray_mesh_ref.cast's distance and geom, the surface normal at the hit and
the FEATURE of the geom the hit lies on, and the colour of a pixel.  It shares no code with the device: the hit comes from
ray_ref / ray_mesh_ref, the normal from the geometry of the hit point, a height field's and a mesh's from a brute-force loop over
every triangle.

cast() returns (dist, geomid, normal [n, 3], feature [n]).  The normal is unit, in the world frame, oriented towards the ray's origin
(n . v <= 0); (0, 0, 0) on a miss.  In the geom's frame, at the hit point h, before orientation: plane (0, 0, 1); sphere h; ellipsoid
h / size^2; capsule h - (0, 0, clamp(h_z, -s1, s1)); cylinder the cap (0, 0, sign h_z) where |h_z| - s1 >= hypot(h_x, h_y) - s0, else
radial; box the axis with the largest |h_i| - s_i, sign of h_i; height field the normal of the top triangle, the wall's or the base's;
mesh the normal of the triangle (of the hull in mesh mode 1, of the mesh itself with the triangle surface).

Features (integers, comparable only within one geom): box 2 axis + (h > 0); cylinder 0 side, 1 / 2 the caps; height field -1 base,
-2 .. -5 the walls, 2 (r (ncol - 1) + c) + k triangle k of cell (r, c); mesh the triangle's index; 0 for the smooth types.  A pixel's
normal is trustworthy where its four shifted rays (ray_ref.robust's shifts) name the same feature, or a normal within 1e-9 of the
centre ray's (coplanar neighbours: the two triangles of a hull's quad): feature_robust()."""
import numpy as np

import ray_mesh_ref as rm
import ray_ref as rr

EDGE_SLACK = 1e-12


def _unit(n):
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    return np.where(ln > 0, n / np.where(ln > 0, ln, 1.0), 0.0)


def _tri_feature(P, V, tris):
    """(x, index, normal) of the nearest triangle hit, two-sided, by brute force; index -1: none"""
    best = np.full(len(P), -1.0); idx = np.full(len(P), -1); nrm = np.zeros((len(P), 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        for k, (a, b, c) in enumerate(np.asarray(tris, float)):
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
            take = ok & ((best < 0) | (x < best))
            best = np.where(take, x, best); idx = np.where(take, k, idx); nrm = np.where(take[:, None], n / np.linalg.norm(n), nrm)
    return best, idx, nrm


def _hfield_feature(P, V, hf):
    """(x, feature, normal) of the nearest surface of the height-field solid: base, walls, then every top triangle"""
    nrow, ncol, size, data = hf
    sx, sy, sz, sb = size
    best = np.full(len(P), -1.0); feat = np.zeros(len(P), int); nrm = np.zeros((len(P), 3))

    def pick(x, ok, f, n):
        nonlocal best, feat, nrm
        take = ok & (x >= 0) & ((best < 0) | (x < best))
        best = np.where(take, x, best); feat = np.where(take, f, feat); nrm = np.where(take[:, None], np.asarray(n, float), nrm)
    with np.errstate(invalid="ignore", divide="ignore"):
        x = (-sb - P[:, 2]) / V[:, 2]
        x = np.where(np.isfinite(x), x, -1.0)
        H = P + x[:, None] * V
        pick(x, (np.abs(H[:, 0]) <= sx) & (np.abs(H[:, 1]) <= sy), -1, (0, 0, -1.0))
        k = 0
        for ax, sa, so in ((0, sx, sy), (1, sy, sx)):
            for w in (-1.0, 1.0):
                x = (w * sa - P[:, ax]) / V[:, ax]
                x = np.where(np.isfinite(x), x, -1.0)
                H = P + x[:, None] * V
                H[:, ax] = w * sa
                ok = (np.abs(H[:, 1 - ax]) <= so) & (H[:, 2] >= -sb) & (H[:, 2] <= rr.hfield_height(hf, H[:, 0], H[:, 1]))
                n = np.zeros(3); n[ax] = w
                pick(x, ok, -2 - k, n)
                k += 1
    z = np.asarray(data) * sz
    xs = -sx + 2 * sx * np.arange(ncol) / (ncol - 1); ys = -sy + 2 * sy * np.arange(nrow) / (nrow - 1)
    tris, ids = [], []
    for r in range(nrow - 1):
        for c in range(ncol - 1):
            a = np.array([xs[c], ys[r], z[r, c]]); d = np.array([xs[c + 1], ys[r + 1], z[r + 1, c + 1]])
            # triangle 0: u >= w (the corner (r, c + 1)); triangle 1: w >= u (the corner (r + 1, c))
            tris.append((a, np.array([xs[c + 1], ys[r], z[r, c + 1]]), d)); ids.append(2 * (r * (ncol - 1) + c))
            tris.append((a, d, np.array([xs[c], ys[r + 1], z[r + 1, c]]))); ids.append(2 * (r * (ncol - 1) + c) + 1)
    tx, ti, tn = _tri_feature(P, V, np.array(tris))
    take = (ti >= 0) & ((best < 0) | (tx < best))
    best = np.where(take, tx, best); feat = np.where(take, np.array(ids)[np.maximum(ti, 0)], feat); nrm = np.where(take[:, None], tn, nrm)
    return best, feat, nrm


def geom_normal(gtype, P, V, x, size, hf=None, tris=None):
    """(normal [n, 3] in the geom frame, not oriented, unit; feature [n]) at the hits P + x V of rays given in the frame of one geom"""
    P = np.asarray(P, float).reshape(-1, 3); V = np.asarray(V, float).reshape(-1, 3)
    H = P + np.asarray(x, float)[:, None] * V
    s = np.asarray(size, float)
    feat = np.zeros(len(P), int)
    if gtype == rr.PLANE:
        n = np.tile([0.0, 0, 1.0], (len(P), 1))
    elif gtype == rr.SPHERE:
        n = H
    elif gtype == rr.ELLIPSOID:
        n = H / (s * s)
    elif gtype == rr.CAPSULE:
        n = H - np.stack([0 * H[:, 2], 0 * H[:, 2], np.clip(H[:, 2], -s[1], s[1])], axis=1)
    elif gtype == rr.CYLINDER:
        cap = np.abs(H[:, 2]) - s[1] >= np.hypot(H[:, 0], H[:, 1]) - s[0]
        n = np.where(cap[:, None], np.stack([0 * H[:, 2], 0 * H[:, 2], np.sign(H[:, 2])], axis=1), H * [1.0, 1.0, 0.0])
        feat = np.where(cap, np.where(H[:, 2] > 0, 1, 2), 0)
    elif gtype == rr.BOX:
        ax = np.argmax(np.abs(H) - s, axis=1)
        sg = np.sign(H[np.arange(len(H)), ax])
        n = np.zeros((len(P), 3)); n[np.arange(len(H)), ax] = sg
        feat = 2 * ax + (sg > 0)
    elif gtype == rr.HFIELD:
        xx, feat, n = _hfield_feature(P, V, hf)
        assert np.allclose(xx, x, rtol=0, atol=1e-9), "the feature search finds ray_ref's distance"
    elif gtype == rr.MESH:
        xx, feat, n = _tri_feature(P, V, tris)
        assert np.allclose(xx, x, rtol=0, atol=1e-9), "the feature search finds ray_mesh_ref's distance"
    else:
        raise ValueError(gtype)
    return _unit(n), feat


def cast(pnt, vec, scene, cutoff=0.0):
    """(dist, geomid, normal, feature) of world-frame rays: ray_mesh_ref.cast's hit, the world-frame unit normal oriented towards the
    origin of the ray, the feature id"""
    P = np.asarray(pnt, float).reshape(-1, 3); V = np.asarray(vec, float).reshape(-1, 3)
    dist, gid = rm.cast(P, V, scene, cutoff)
    nrm = np.zeros((len(P), 3)); feat = np.zeros(len(P), int)
    for g in np.unique(gid[gid >= 0]):
        k = np.nonzero(gid == g)[0]
        t = int(scene["type"][g])
        R = np.asarray(scene["mat"][g], float).reshape(3, 3)
        lp = (P[k] - scene["pos"][g]) @ R; lv = V[k] @ R
        n, f = geom_normal(t, lp, lv, dist[k], scene["size"][g], scene.get("hfield", {}).get(g), scene.get("mesh", {}).get(g))
        nw = n @ R.T
        flip = np.sum(nw * V[k], axis=1) > 0
        nrm[k] = np.where(flip[:, None], -nw, nw); feat[k] = f
    return dist, gid, nrm, feat


def shifted(rays, shift=1e-4):
    """the four shifted ray sets of ray_ref.robust: +-shift along two directions perpendicular to each ray"""
    P = np.asarray(rays[0], float).reshape(-1, 3); V = np.asarray(rays[1], float).reshape(-1, 3)
    u = V / np.linalg.norm(V, axis=1, keepdims=True)
    helper = np.where(np.abs(u[:, [0]]) < 0.9, np.array([[1.0, 0, 0]]), np.array([[0, 1.0, 0]]))
    e1 = np.cross(u, helper); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(u, e1)
    return [(P + s * e, V) for e in (e1, e2) for s in (shift, -shift)]


def robust_both(rays, scene, centre=None, tol=1e-3, ntol=1e-9):
    """(robust, feature-robust) [nray]: ray_ref.robust's rule (same geom, distance within tol at the four shifts), and: at the four
    shifts the same feature, or a normal within ntol of the centre ray's"""
    d0, g0, n0, f0 = centre if centre is not None else cast(rays[0], rays[1], scene)
    rob = np.ones(len(d0), bool); frob = np.ones(len(d0), bool)
    for P, V in shifted(rays):
        d, g, n, f = cast(P, V, scene)
        rob &= (g == g0) & (np.abs(d - d0) <= tol)
        frob &= (f == f0) | (np.abs(n - n0).max(axis=1) <= ntol)
    return rob, frob


def level(c):
    """(int)(255 min(1, c) + 0.5) in float32, the product and the sum rounded separately"""
    c = np.minimum(np.float32(1.0), np.asarray(c, np.float32))
    return ((np.float32(255.0) * c).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.int64)


def colour(rgba, gid, normal, vec, ambient=0.3, diffuse=0.7, background=(0.0, 0.0, 0.0, 0.0)):
    """uint8 [n, 4]: R, G, B = level(geom_rgba[g][c] shade) with shade = ambient + diffuse |n . v^| in float32, A = 255; a miss is
    level(background)"""
    rgba = np.asarray(rgba, float).reshape(-1, 4)
    V = np.asarray(vec, float).reshape(-1, 3)
    ndv = np.abs(np.sum(normal * V, axis=1)) / np.linalg.norm(V, axis=1)
    shade = (np.float32(ambient) + (np.float32(diffuse) * np.minimum(ndv, 1.0).astype(np.float32)).astype(np.float32)).astype(np.float32)
    out = np.tile(level(np.asarray(background, np.float32)), (len(V), 1))
    hit = gid >= 0
    col = rgba[np.maximum(gid, 0)].astype(np.float32)
    rgb = level((col[:, :3] * shade[:, None]).astype(np.float32))
    out[hit, :3] = rgb[hit]; out[hit, 3] = 255
    return out.astype(np.uint8)
