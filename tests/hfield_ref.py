"""Reference for the height-field narrow phase: the prism enumeration restated in numpy, each prism's contact
from the frozen oracle's fp64 portal refinement (orc_convex_pair with the prism as a 6-vertex mesh placed at its vertex mean).

The choices restated here are the kernel's own (step_kernel.h, hfield_pair): the cells the other geom's bounding sphere covers,
widened by the margin; corners (r, c), (r+1, c+1) and then (r, c+1) for the first triangle of a cell, (r+1, c) for the second;
prisms in the order row, column, triangle; a prism whose three tops lie below the geom's lowest bounding-sphere point minus the
margin is skipped; one contact per prism, the first MAXCON of a pair kept.  The oracle has no hfield routine of its own, so
no OrcData is ever built on an hfield model."""
import ctypes as C

import numpy as np

import orc

MAXCON = 50
GEOM_MESH = 7


def hfield_of(m, g):
    """(nrow, ncol, size[4], normalised elevation [nrow, ncol]) of hfield geom g"""
    h = int(m.array("geom_dataid")[g])
    nrow, ncol = int(m.array("hfield_nrow")[h]), int(m.array("hfield_ncol")[h])
    adr = int(m.array("hfield_adr")[h])
    size = m.array("hfield_size")[4 * h:4 * h + 4]
    data = m.array("hfield_data")[adr:adr + nrow * ncol].reshape(nrow, ncol)
    return nrow, ncol, size, data


def grid_xy(nrow, ncol, size, r, c):
    return -size[0] + 2 * size[0] * c / (ncol - 1), -size[1] + 2 * size[1] * r / (nrow - 1)


def prisms(nrow, ncol, size, data, lp, rbound, margin):
    """prisms a geom whose centre is lp (hfield frame) and bounding radius rbound may touch, in the kernel's order:
    list of (r, c, tri, verts[6, 3]) with the three tops first, then the three bottoms (hfield frame)"""
    R = rbound + margin
    if (lp[0] + R < -size[0] or lp[0] - R > size[0] or lp[1] + R < -size[1] or lp[1] - R > size[1]
            or lp[2] - R > size[2] or lp[2] + R < -size[3]):
        return []
    dx, dy = 2 * size[0] / (ncol - 1), 2 * size[1] / (nrow - 1)
    clamp = lambda v, hi: int(min(max(np.floor(v), 0), hi))
    c0, c1 = clamp((lp[0] - R + size[0]) / dx, ncol - 2), clamp((lp[0] + R + size[0]) / dx, ncol - 2)
    r0, r1 = clamp((lp[1] - R + size[1]) / dy, nrow - 2), clamp((lp[1] + R + size[1]) / dy, nrow - 2)
    low = lp[2] - rbound - margin
    out = []
    for r in range(r0, r1 + 1):
        for c in range(c0, c1 + 1):
            for tri in (0, 1):
                corners = [(r, c), (r + 1, c + 1), (r + 1, c) if tri else (r, c + 1)]
                tops = [data[a, b] * size[2] for a, b in corners]
                if max(tops) < low:
                    continue
                v = np.zeros((6, 3))
                for i, (a, b) in enumerate(corners):
                    x, y = grid_xy(nrow, ncol, size, a, b)
                    v[i] = (x, y, tops[i]); v[3 + i] = (x, y, -size[3])
                out.append((r, c, tri, v))
    return out


def _dp(a):
    return np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(C.POINTER(C.c_double))


def expected_contacts(m, hg, og, gpos, gmat, maxcon=MAXCON):
    """contacts of the pair (hfield geom hg, geom og) at world poses gpos [ngeom, 3], gmat [ngeom, 9], in prism order, capped:
    list of dicts dist, pos[3], normal[3] (from the terrain into og), prism (r, c, tri)"""
    L = orc.lib()
    nrow, ncol, size, data = hfield_of(m, hg)
    margin = max(float(m.array("geom_margin")[hg]), float(m.array("geom_margin")[og]))
    p1, m1 = np.asarray(gpos[hg], float), np.asarray(gmat[hg], float).reshape(3, 3)
    p2, m2 = np.asarray(gpos[og], float), np.asarray(gmat[og], float).reshape(3, 3)
    lp = m1.T @ (p2 - p1)
    t2 = int(m.array("geom_type")[og])
    s2 = m.array("geom_size")[3 * og:3 * og + 3]
    v2, n2 = np.zeros(3), 0
    if t2 == GEOM_MESH:
        mid = int(m.array("geom_dataid")[og])
        a, n2 = int(m.array("mesh_vertadr")[mid]), int(m.array("mesh_vertnum")[mid])
        v2 = m.array("mesh_vert")[3 * a:3 * (a + n2)]
    out = []
    for r, c, tri, v in prisms(nrow, ncol, size, data, lp, float(m.array("geom_rbound")[og]), margin):
        ctr = v.mean(axis=0)
        rel = v - ctr
        cw = p1 + m1 @ ctr
        dist, pos, nrm = C.c_double(), np.zeros(3), np.zeros(3)
        n = L.orc_convex_pair(GEOM_MESH, _dp(cw), _dp(m1.ravel()), _dp(np.zeros(3)), _dp(rel.ravel()), 6,
                              t2, _dp(p2), _dp(m2.ravel()), _dp(s2), _dp(v2), n2, margin,
                              C.byref(dist), pos.ctypes.data_as(C.POINTER(C.c_double)), nrm.ctypes.data_as(C.POINTER(C.c_double)))
        if n:
            out.append(dict(dist=dist.value, pos=pos.copy(), normal=nrm.copy(), prism=(r, c, tri)))
            if len(out) == maxcon:
                break
    return out
