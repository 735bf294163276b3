"""fp64 numpy reference for 2D textures in the colour image (mjh_render_set_texturing 1; include/mjhip.h holds the definitions).  It
shares no code with the device or the builder: the builtin generators and the mapping are written from the definitions, the hit of a
pixel comes from render_ref.cast, the light terms from light_ref.terms.

A texture is a uint8 array [H, W, 3], row 0 first.  A geom's texture record is a dict tex (index into the texture list, -1 none),
repeat (rx, ry), uniform (bool).

builtin():  a byte is (int)(255 c + 0.5); flat rgb1; checker rgb1 where (j < H // 2) == (i < W // 2), rgb2 elsewhere; gradient
rgb1 (1 - r) + rgb2 r with r = min(1, hypot(x, y)), x = 2 i / (W - 1) - 1, y = 2 j / (H - 1) - 1 (0 where the dimension is 1); mark
edge: row 0, row H - 1, column 0, column W - 1 take markrgb; mark cross: row H // 2 and column W // 2.

texel_index():  X = h_x / a_x, Y = h_y / a_y with a = (1, 1) for a uniform texture, else the half extents of the geom in x and y
(plane size[0..1], 0 counting as 1; box, ellipsoid size[0..1]; sphere, capsule, cylinder (r, r); height field hfield_size[0..1]);
u = 0.5 rx X + 0.5, v = 0.5 - 0.5 ry Y; column min(W - 1, floor((u - floor u) W)), row the same from v and H."""
import numpy as np

import ray_ref as rr
import render_ref as rf

FLAT, CHECKER, GRADIENT = 0, 1, 2
NONE, EDGE, CROSS = 0, 1, 2


def byte(c):
    return (255.0 * np.asarray(c, float) + 0.5).astype(int)


def builtin(kind, width, height, rgb1=(0.8, 0.8, 0.8), rgb2=(0.5, 0.5, 0.5), mark=NONE, markrgb=(0.0, 0.0, 0.0)):
    W, H = int(width), int(height)
    j, i = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    if kind == FLAT:
        r = np.zeros((H, W))
    elif kind == CHECKER:
        r = np.where((j < H // 2) == (i < W // 2), 0.0, 1.0)
    elif kind == GRADIENT:
        x = 2.0 * i / (W - 1) - 1.0 if W > 1 else np.zeros((H, W))
        y = 2.0 * j / (H - 1) - 1.0 if H > 1 else np.zeros((H, W))
        r = np.minimum(1.0, np.sqrt(x * x + y * y))
    else:
        raise ValueError(kind)
    out = byte(np.asarray(rgb1, float) * (1.0 - r[..., None]) + np.asarray(rgb2, float) * r[..., None])
    if mark == EDGE:
        m = (j == 0) | (j == H - 1) | (i == 0) | (i == W - 1)
    elif mark == CROSS:
        m = (j == H // 2) | (i == W // 2)
    else:
        m = np.zeros((H, W), bool)
    out[m] = byte(markrgb)
    return out.astype(np.uint8)


def extents(gtype, size, uniform, hfield_size=None):
    """the half extents (a_x, a_y) the mapping divides by"""
    if uniform:
        return 1.0, 1.0
    s = np.asarray(size, float)
    if gtype == rr.PLANE:
        return (s[0] if s[0] > 0 else 1.0), (s[1] if s[1] > 0 else 1.0)
    if gtype == rr.HFIELD:
        return float(hfield_size[0]), float(hfield_size[1])
    if gtype in (rr.SPHERE, rr.CAPSULE, rr.CYLINDER):
        return s[0], s[0]
    if gtype in (rr.BOX, rr.ELLIPSOID):
        return s[0], s[1]
    raise ValueError(gtype)


def texel_index(h, a, repeat, width, height):
    """(row, column) of hit points h [n, 3] given in the geom's frame"""
    h = np.asarray(h, float).reshape(-1, 3)
    u = 0.5 * repeat[0] * (h[:, 0] / a[0]) + 0.5
    v = 0.5 - 0.5 * repeat[1] * (h[:, 1] / a[1])
    col = np.minimum(width - 1, np.floor((u - np.floor(u)) * width).astype(int))
    row = np.minimum(height - 1, np.floor((v - np.floor(v)) * height).astype(int))
    return row, col


def texels(textures, records, scene, gid, hits):
    """(bytes [n, 3] int, textured [n] bool) of world-frame hit points `hits` on geoms `gid` (-1: a miss) of `scene`"""
    gid = np.asarray(gid); hits = np.asarray(hits, float).reshape(-1, 3)
    out = np.zeros((len(gid), 3), int); has = np.zeros(len(gid), bool)
    for g in np.unique(gid[gid >= 0]):
        R = records[int(g)]
        if R["tex"] < 0:
            continue
        k = np.nonzero(gid == g)[0]
        T = np.asarray(textures[R["tex"]])
        M = np.asarray(scene["mat"][g], float).reshape(3, 3)
        h = (hits[k] - scene["pos"][g]) @ M
        hf = scene.get("hfield", {}).get(int(g))
        a = extents(int(scene["type"][g]), scene["size"][g], R["uniform"], None if hf is None else hf[2])
        row, col = texel_index(h, a, R["repeat"], T.shape[1], T.shape[0])
        out[k] = T[row, col]; has[k] = True
    return out, has


def albedo(colours, textures, records, scene, gid, hits):
    """[n, 4] the base colour of every pixel: geom_rgba[g], its r, g, b times texel / 255 where the geom carries a texture (float32
    quotient and product, as the definition states them); rows of misses are zero"""
    gid = np.asarray(gid)
    col = np.asarray(colours, float).reshape(-1, 4)[np.maximum(gid, 0)].astype(np.float32)
    t, has = texels(textures, records, scene, gid, hits)
    q = (t.astype(np.float32) / np.float32(255.0)).astype(np.float32)
    col[:, :3] = np.where(has[:, None], (col[:, :3] * q).astype(np.float32), col[:, :3])
    col[gid < 0] = 0.0
    return col.astype(float)


def hit_points(rays, dist, gid):
    P = np.asarray(rays[0], float).reshape(-1, 3); V = np.asarray(rays[1], float).reshape(-1, 3)
    return P + np.where(np.asarray(gid) >= 0, dist, 0.0)[:, None] * V
