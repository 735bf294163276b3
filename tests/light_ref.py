"""fp64 numpy reference for lights and cast shadows in the colour image (mjh_render_set_lighting 1; include/mjhip.h holds the
definition).  It shares no code with the device: the hit and the normal of a pixel come from render_ref.cast, the light terms from the
definition, the shadow rays go through ray_mesh_ref.cast.

A light is a dict in the WORLD frame: pos [3], dir [3] (unit), directional, castshadow (bools), diffuse [3], ambient [3], cutoff
(degrees), exponent.  world_lights() makes them from a model's light_* arrays and body poses.

terms() returns, per light, amb_l + dif_l t_l [nl, npix, 3] with t_l = max(0, n . l^) spot lit, and the mask of pixels in CAST shadow
[nl, npix]: n . l^ > 0, spot > 0 and the shadow ray blocked (a pixel that faces away from the light is not counted: it loses nothing).
The shadow ray starts at o = h + bias n; a directional light's runs along -d^ without bound, a positional light's along L - o and only
a hit with parameter < 1 blocks it."""
import numpy as np

import ray_mesh_ref as rm
import ray_ref as rr
import render_ref as rf


def world_lights(m, xpos, xquat, active=None):
    """the model's lights (light_active, or `active` [nlight] in its place) in the world frame of body poses xpos [nbody, 3], xquat [nbody, 4]"""
    nl = m.nlight
    body = m.array("light_bodyid")
    pos, dr = m.array("light_pos").reshape(-1, 3), m.array("light_dir").reshape(-1, 3)
    on = m.array("light_active") if active is None else np.asarray(active)
    out = []
    for l in range(nl):
        if not on[l]:
            continue
        R = rr.quat2mat(np.asarray(xquat, float)[body[l]]).reshape(3, 3)
        out.append(dict(pos=np.asarray(xpos, float)[body[l]] + R @ pos[l], dir=R @ dr[l], directional=bool(m.array("light_directional")[l]),
                        castshadow=bool(m.array("light_castshadow")[l]), diffuse=m.array("light_diffuse").reshape(-1, 3)[l],
                        ambient=m.array("light_ambient").reshape(-1, 3)[l], cutoff=float(m.array("light_cutoff")[l]),
                        exponent=float(m.array("light_exponent")[l])))
    return out


def f32_lights(lights):
    """the lights with every number rounded to float32 (what the host build is given)"""
    f = lambda x: np.asarray(x, np.float32).astype(float)
    return [dict(L, pos=f(L["pos"]), dir=f(L["dir"]), diffuse=f(L["diffuse"]), ambient=f(L["ambient"]), exponent=float(np.float32(L["exponent"]))) for L in lights]


def terms(lights, rays, scene, centre=None, bias=1e-3, shadows=True):
    """(term [nl, npix, 3], cast-shadow mask [nl, npix]) for the pixels of `rays`; centre: render_ref.cast of the rays"""
    P = np.asarray(rays[0], float).reshape(-1, 3); V = np.asarray(rays[1], float).reshape(-1, 3)
    dist, gid, n, _ = centre if centre is not None else rf.cast(P, V, scene)
    hit = gid >= 0
    h = P + np.where(hit, dist, 0.0)[:, None] * V
    o = h + bias * n
    term = np.zeros((len(lights), len(P), 3)); cast = np.zeros((len(lights), len(P)), bool)
    for k, L in enumerate(lights):
        d = np.asarray(L["dir"], float)
        if L["directional"]:
            lhat = np.tile(-d, (len(P), 1)); spot = np.ones(len(P)); sv = lhat.copy()
        else:
            l = np.asarray(L["pos"], float) - h
            ln = np.linalg.norm(l, axis=1)
            lhat = l / np.where(ln > 0, ln, 1.0)[:, None]
            c = -(lhat @ d)
            inside = (c >= np.cos(np.radians(L["cutoff"]))) & (c > 0) & (ln > 0)
            spot = np.where(inside, np.power(np.where(inside, c, 1.0), L["exponent"]), 0.0)
            sv = np.asarray(L["pos"], float) - o
        ndl = np.sum(n * lhat, axis=1)
        lit = np.ones(len(P))
        if shadows and L["castshadow"]:
            need = np.nonzero(hit & (ndl > 0) & (spot > 0))[0]
            if len(need):
                sd, sg = rm.cast(o[need], sv[need], scene)
                blocked = (sg >= 0) & (True if L["directional"] else (sd < 1.0))
                lit[need[blocked]] = 0.0
                cast[k, need[blocked]] = True
        t = np.maximum(ndl, 0.0) * spot * lit
        term[k] = np.where(hit[:, None], np.asarray(L["ambient"], float) + np.asarray(L["diffuse"], float) * t[:, None], 0.0)
    return term, cast


def colour(rgba, gid, normal, vec, term, ambient=0.3, diffuse=0.7, background=(0.0, 0.0, 0.0, 0.0)):
    """uint8 [n, 4]: R, G, B = level(geom_rgba[g][c] (shade + sum_l term_l[c])) in float32 with render_ref's shade, A = 255; a miss is
    level(background)"""
    rgba = np.asarray(rgba, float).reshape(-1, 4)
    V = np.asarray(vec, float).reshape(-1, 3)
    ndv = np.abs(np.sum(normal * V, axis=1)) / np.linalg.norm(V, axis=1)
    shade = (np.float32(ambient) + (np.float32(diffuse) * np.minimum(ndv, 1.0).astype(np.float32)).astype(np.float32)).astype(np.float32)
    total = np.zeros((len(V), 3), np.float32)
    for t in np.asarray(term, float):
        total = (total + t.astype(np.float32)).astype(np.float32)
    out = np.tile(rf.level(np.asarray(background, np.float32)), (len(V), 1))
    hit = gid >= 0
    col = rgba[np.maximum(gid, 0)].astype(np.float32)
    rgb = rf.level((col[:, :3] * (shade[:, None] + total).astype(np.float32)).astype(np.float32))
    out[hit, :3] = rgb[hit]; out[hit, 3] = 255
    return out.astype(np.uint8)
