"""Height fields on the device: the prism narrow phase against the numpy / oracle reference (hfield_ref.py), resting and
sliding on terrain against the same scene on a plane, every layout and launch form, the 50-contact cap and the capacity flag,
and a soak."""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
import hfield_ref
from helpers import D, set_opt

pytestmark = pytest.mark.gpu

PLANE, HFIELD, SPHERE, CAPSULE, ELLIPSOID, CYLINDER, BOX, MESH = range(8)
SHAPES = [(SPHERE, (0.07, 0, 0)), (CAPSULE, (0.05, 0.08, 0)), (BOX, (0.08, 0.06, 0.05)), (CYLINDER, (0.06, 0.05, 0)),
          (ELLIPSOID, (0.08, 0.06, 0.05)), (MESH, None)]


def _quat_z(a):
    return (np.cos(a / 2), 0, 0, np.sin(a / 2))


def _terrain_elev(rng, nrow, ncol):
    x, y = np.meshgrid(np.linspace(0, 1, ncol), np.linspace(0, 1, nrow))
    e = np.sin(6 * x + rng.uniform(0, 6)) * np.cos(5 * y + rng.uniform(0, 6)) + 0.3 * rng.normal(size=(nrow, ncol))
    return e.ravel()


def _model(lib, elev, nrow, ncol, size, shapes=SHAPES, hpos=(0, 0, 0), hquat=None, capacity=None, plane_at=None,
           friction=None, timestep=0.002, tilt=None, arm=False):
    """terrain (or, plane_at = z: a plane instead) + one free body per shape"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=timestep)
    if capacity:
        lib.mjh_builder_set_capacity(b, *capacity)
    fr = D(*friction) if friction else None
    q = tilt if tilt is not None else hquat
    if plane_at is None:
        e = (C.c_double * len(elev))(*elev)
        h = lib.mjh_builder_add_hfield(b, b"terrain", nrow, ncol, D(*size), e)
        assert lib.mjh_builder_add_hfield_geom(b, b"ground", 0, h, D(*hpos), D(*q) if q is not None else None, fr, -1, -1, -1) >= 0
    else:
        lib.mjh_builder_add_geom(b, b"ground", 0, PLANE, D(5, 5, 0.1), D(0, 0, plane_at), D(*q) if q is not None else None, fr, -1, -1, -1, -1)
    for k, (t, s) in enumerate(shapes):
        bd = lib.mjh_builder_add_body(b, b"b%d" % k, 0, D(0.3 * k - 0.6, 0, 1.0), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        if t == MESH:
            v = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], float) * [0.07, 0.05, 0.04]
            v = np.vstack([v, [[0, 0, 0.08], [0.09, 0, 0]]])
            vv = np.ascontiguousarray(v)
            mid = lib.mjh_builder_add_mesh(b, vv.ctypes.data_as(C.POINTER(C.c_double)), len(vv), None, 0, None)
            assert mid >= 0
            assert lib.mjh_builder_add_mesh_geom(b, b"g%d" % k, bd, mid, None, None, fr, -1, -1, -1, -1) >= 0
        else:
            lib.mjh_builder_add_geom(b, b"g%d" % k, bd, t, D(*s), None, None, fr, -1, -1, -1, -1)
    if arm:      # a two-link arm on a hinge base whose tip sphere reaches the terrain
        a1 = lib.mjh_builder_add_body(b, b"arm1", 0, D(0.0, 0.5, 0.5), None, 0.0)
        lib.mjh_builder_add_joint(b, b"h1", a1, 3, D(0, 0, 0), D(0, 1, 0), None, 0.5, 0, 0, 0, 0)
        lib.mjh_builder_add_geom(b, b"l1", a1, CAPSULE, D(0.03, 0.15, 0), D(0.15, 0, 0), D(0.7071068, 0, 0.7071068, 0), None, 0, 0, -1, -1)
        a2 = lib.mjh_builder_add_body(b, b"arm2", a1, D(0.3, 0, 0), None, 0.0)
        lib.mjh_builder_add_joint(b, b"h2", a2, 3, D(0, 0, 0), D(0, 1, 0), None, 0.5, 0, 0, 0, 0)
        lib.mjh_builder_add_geom(b, b"tip", a2, SPHERE, D(0.06, 0, 0), D(0.3, 0, 0), None, None, -1, -1, -1, -1)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    return m


def _surface(m, hg, gpos, gmat, xy):
    """terrain height (world z) under world point xy, from the triangles of the cell (flat geom frame only used for checks)"""
    nrow, ncol, size, data = hfield_ref.hfield_of(m, hg)
    R = np.asarray(gmat, float).reshape(3, 3)
    lp = R.T @ (np.array([xy[0], xy[1], 0.0]) - gpos)
    fx = np.clip((lp[0] + size[0]) / (2 * size[0]) * (ncol - 1), 0, ncol - 1 - 1e-9)
    fy = np.clip((lp[1] + size[1]) / (2 * size[1]) * (nrow - 1), 0, nrow - 1 - 1e-9)
    c, r = int(fx), int(fy); u, v = fx - c, fy - r
    z = data * size[2]
    if v <= u:   # triangle (r,c), (r+1,c+1), (r,c+1)
        h = z[r, c] + u * (z[r, c + 1] - z[r, c]) + v * (z[r + 1, c + 1] - z[r, c + 1])
    else:        # triangle (r,c), (r+1,c+1), (r+1,c)
        h = z[r, c] + v * (z[r + 1, c] - z[r, c]) + u * (z[r + 1, c + 1] - z[r + 1, c])
    return gpos[2] + h


def _random_poses(m, rng, nenv, hg, gpos_h, gmat_h, spread):
    nb = len(SHAPES)
    q = np.zeros((nenv, m.nq))
    for i in range(nenv):
        for k in range(nb):
            xy = rng.uniform(-spread, spread, size=2) + gpos_h[:2]
            z = _surface(m, hg, gpos_h, gmat_h, xy) + rng.uniform(-0.01, 0.12)
            quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
            q[i, 7 * k:7 * k + 3] = (xy[0], xy[1], z); q[i, 7 * k + 3:7 * k + 7] = quat
    return q


def test_contacts_match_reference(lib):
    """every (hfield, geom) pair of 256 random envs: the device's contacts are the reference's, in the same order"""
    rng = np.random.default_rng(7)
    nrow, ncol = 24, 20
    cases = [(0.05, (0, 0, 0), None), (0.2, (0, 0, 0), None), (0.45, (0.3, -0.2, 0.1), _quat_z(0.6))]
    npairs = nmis = nsoft = ncon = nfar = 0
    for amp, hpos, hq in cases:
        m = _model(lib, _terrain_elev(rng, nrow, ncol), nrow, ncol, (1.2, 1.0, amp, 0.3), hpos=hpos, hquat=hq)
        hg = m.name2id(2, "ground")
        nenv = 256
        e = ms.Engine(m, nenv)
        gp0, gm0 = e.get_geom_state(0, 1)
        q = _random_poses(m, rng, nenv, hg, gp0[0, hg], gm0[0, hg], 0.75)
        e.set_initial_qpos(q); e.reset(); e.forward(); e.synchronize()
        gpos, gmat = e.get_geom_state()
        for i in range(nenv):
            c = e.get_contacts(i)
            for og in range(m.ngeom):
                if og == hg:
                    continue
                ref = hfield_ref.expected_contacts(m, hg, og, gpos[i], gmat[i])
                dev = [k for k, g in enumerate(c["geom"]) if g[0] == hg and g[1] == og]
                if not ref and not dev:
                    continue
                npairs += 1
                if len(ref) != len(dev):
                    # a grazing prism may fall either side in fp32: every contact that only one side has lies within 2e-4 of the
                    # margin, so the firm ones are the same contacts in the same order
                    firm_r = [x for x in ref if x["dist"] < -2e-4]
                    firm_d = [k for k in dev if c["dist"][k] < -2e-4]
                    assert len(firm_r) == len(firm_d), (amp, i, og, len(ref), len(dev))
                    for x, k in zip(firm_r, firm_d):
                        assert abs(c["dist"][k] - x["dist"]) < 5e-3 or x["dist"] < -0.01, (amp, i, og)
                    nmis += 1
                    continue
                for x, k in zip(ref, dev):
                    if x["dist"] < -0.01:       # (deeper: the fp32 and fp64 refinements of the tall prisms take different portals)
                        continue
                    ncon += 1
                    # (the fp32 refinement can stop on another portal of a tall, narrow prism than the fp64 one: counted, bounded below)
                    if abs(c["dist"][k] - x["dist"]) >= 3e-4:
                        nfar += 1
                        assert abs(c["dist"][k] - x["dist"]) < 5e-3, (amp, i, og, m.array("geom_type")[og], c["dist"][k], x["dist"])
                    if np.abs(c["frame"][k][:3] - x["normal"]).max() > 0.05 or np.abs(c["pos"][k] - x["pos"]).max() > 5e-3:
                        nsoft += 1
        e.close()
    assert npairs >= 500 and ncon >= 1000, (npairs, ncon)
    print(f"hfield pairs {npairs}, mismatched {nmis}, contacts {ncon}, normal/pos outside {nsoft}, dist beyond 3e-4 {nfar}")
    assert nmis <= 0.05 * npairs and nsoft <= 0.15 * ncon and nfar <= 0.02 * ncon, (npairs, nmis, ncon, nsoft, nfar)


def test_rest_on_flat_terrain_matches_plane(lib):
    """bodies dropped at random places and headings on a flat terrain at height h settle at the height they reach on a plane at h.
    Box and cylinder come to rest.  Sphere, capsule and ellipsoid do NOT: one contact per prism, and where the body's lowest point
    is near a cell's edge or diagonal, the neighbouring prism's contact comes through its side wall with a tilted normal; they keep
    rolling at a few cm/s (measured: at most 5.5 cm/s and 1.4 rad/s after 2 s, 5.1 cm/s and 1.2 rad/s after 5 s).  The bounds
    below hold that measurement and require that the creep does not grow; it is a known limit of the prism model."""
    shapes = [(SPHERE, (0.07, 0, 0)), (BOX, (0.08, 0.06, 0.05)), (CYLINDER, (0.06, 0.05, 0)), (ELLIPSOID, (0.08, 0.06, 0.05)),
              (CAPSULE, (0.05, 0.08, 0))]
    h = 0.25
    mh = _model(lib, np.zeros(31 * 31), 31, 31, (1.5, 1.5, 0.2, 0.3), shapes=shapes, hpos=(0, 0, h))
    mp = _model(lib, None, 0, 0, None, shapes=shapes, plane_at=h)
    rng = np.random.default_rng(5)
    nenv = 16
    q = np.tile(mh.array("qpos0"), (nenv, 1))
    lying = (0.7071068, 0.7071068, 0, 0)          # the capsule on its side
    for i in range(nenv):
        for k in range(len(shapes)):
            xy = (-1.0 + 0.5 * k + rng.uniform(-0.15, 0.15), rng.uniform(-1.0, 1.0))
            yaw = _quat_z(rng.uniform(0, 2 * np.pi))
            qq = yaw if shapes[k][0] != CAPSULE else tuple(_qmul(yaw, lying))
            q[i, 7 * k:7 * k + 3] = (*xy, h + 0.2); q[i, 7 * k + 3:7 * k + 7] = qq
    out = []
    for m in (mh, mp):
        e = ms.Engine(m, nenv)
        e.set_initial_qpos(q); e.reset(); e.step(1000); e.synchronize()
        _, q2, v2, _ = e.get_state()
        e.step(1500); e.synchronize()
        _, q5, v5, _ = e.get_state()
        e.close()
        w2, w5 = (np.abs(v).reshape(nenv, len(shapes), 6) for v in (v2, v5))
        print("REST", "terrain" if m is mh else "plane", "lin 2s / 5s", w2[:, :, :3].max(axis=(0, 2)).round(5).tolist(), w5[:, :, :3].max(axis=(0, 2)).round(5).tolist(),
              "ang 2s / 5s", w2[:, :, 3:].max(axis=(0, 2)).round(5).tolist(), w5[:, :, 3:].max(axis=(0, 2)).round(5).tolist())
        assert np.isfinite(v5).all()
        if m is mh:
            flat, rnd = [1, 2], [0, 3, 4]          # box, cylinder | sphere, ellipsoid, capsule
            assert w2[:, flat, :3].max() < 1e-3 and w5[:, flat, :3].max() < 1e-3 and w5[:, flat, 3:].max() < 1e-2
            assert w5[:, rnd, :3].max() < 0.08 and w5[:, rnd, 3:].max() < 2.0
            assert w5[:, rnd].max() <= 1.05 * w2[:, rnd].max()          # the creep does not grow
        out.append(q5)
    for k in range(len(shapes)):
        np.testing.assert_allclose(out[0][:, 7 * k + 2], out[1][:, 7 * k + 2], atol=1e-3, err_msg=str(shapes[k]))


def _qmul(a, b):
    w1, x1, y1, z1 = a; w2, x2, y2, z2 = b
    return (w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
            w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2)


def test_incline_matches_tilted_plane(lib):
    """a planar tilted terrain against the same tilt as a plane: sliding box, sticking box, rolling sphere"""
    th = np.deg2rad(15.0)
    tilt = (np.cos(th / 2), 0, np.sin(th / 2), 0)     # about y: the slope descends towards +x
    down = np.array([np.cos(th), 0, -np.sin(th)])      # R e_x
    nrow = ncol = 40
    res = {}
    for mu, name in ((0.15, "slide"), (0.6, "stick")):
        shapes = [(BOX, (0.05, 0.05, 0.05)), (SPHERE, (0.05, 0, 0))]
        for kind in ("hf", "plane"):
            if kind == "hf":
                m = _model(lib, np.zeros(nrow * ncol), nrow, ncol, (2.0, 2.0, 0.1, 0.3), shapes=shapes, tilt=tilt, friction=(mu, 0.005, 0.0001))
            else:
                m = _model(lib, None, 0, 0, None, shapes=shapes, plane_at=0.0, tilt=tilt, friction=(mu, 0.005, 0.0001))
            R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
            q = m.array("qpos0").copy()
            for k, (t, s) in enumerate(shapes):
                p = R @ np.array([-1.5, 0.5 * k - 0.25, s[0] if t == SPHERE else s[2]])
                q[7 * k:7 * k + 3] = p; q[7 * k + 3:7 * k + 7] = tilt
            e = ms.Engine(m, 2)
            e.set_initial_qpos(np.tile(q, (2, 1))); e.reset(); e.step(50); e.synchronize()
            _, q0, v0, _ = e.get_state()
            e.step(500); e.synchronize()     # 1 s
            _, q1, v1, _ = e.get_state()
            assert np.isfinite(q1).all()
            res[(name, kind)] = (q0[0], v0[0], q1[0], v1[0])
            e.close()
    g = 9.81
    for kind in ("hf", "plane"):
        q0, v0, q1, v1 = res[("slide", kind)]
        a_box = (v1[0:3] - v0[0:3]) @ down / 1.0
        a_sph = (v1[6:9] - v0[6:9]) @ down / 1.0
        res[("a", kind)] = a_box
        assert a_sph == pytest.approx(5 / 7 * g * np.sin(th), rel=0.02)
        qs0, _, qs1, _ = res[("stick", kind)]
        assert np.linalg.norm(qs1[0:3] - qs0[0:3]) < 1e-3
    assert res[("a", "hf")] == pytest.approx(res[("a", "plane")], rel=0.02)
    assert res[("a", "hf")] > 0.5          # it slides, across many 0.1 m cells
    q0, _, q1, _ = res[("slide", "hf")]
    assert np.linalg.norm(q1[0:3] - q0[0:3]) > 0.5


def _run_form(m, nenv, q, steps, cohorts):
    e = ms.Engine(m, nenv)
    if cohorts > 1:
        e.set_cohorts(cohorts)
    e.set_initial_qpos(q); e.reset(); e.step(steps); e.synchronize()
    _, qq, vv, _ = e.get_state()
    st = e.get_stats()
    gpos, gmat = e.get_geom_state()
    e.close()
    return qq, vv, st, gpos, gmat


_DIRS = [np.array([np.cos(a) * np.sin(b), np.sin(a) * np.sin(b), -np.cos(b)]) for b in (0.0, 0.5, 1.0, 1.4)
         for a in (np.arange(8) * np.pi / 4 if b > 0 else [0.0])]


def _surface_points(m, g, p, R):
    """points on geom g's surface (world): support points along 25 directions of the lower hemisphere, every box corner,
    every mesh vertex"""
    t, s = int(m.array("geom_type")[g]), m.array("geom_size")[3 * g:3 * g + 3]
    if t == MESH:
        mid = int(m.array("geom_dataid")[g]); a, n = int(m.array("mesh_vertadr")[mid]), int(m.array("mesh_vertnum")[mid])
        return p + m.array("mesh_vert")[3 * a:3 * (a + n)].reshape(n, 3) @ R.T
    if t == BOX:
        return p + np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]) * s @ R.T
    pts = []
    for d in _DIRS:
        dl = R.T @ d
        if t == SPHERE:
            pl = s[0] * dl
        elif t == CAPSULE:
            pl = s[0] * dl + [0, 0, s[1] if dl[2] >= 0 else -s[1]]
        elif t == CYLINDER:
            r2 = np.hypot(dl[0], dl[1])
            pl = np.array([s[0] * dl[0] / r2 if r2 > 1e-9 else 0, s[0] * dl[1] / r2 if r2 > 1e-9 else 0, s[1] if dl[2] >= 0 else -s[1]])
        else:
            w = s ** 2 * dl; pl = w / np.sqrt(w @ dl)
        pts.append(p + R @ pl)
    return np.array(pts)


def _check_above(m, gpos, gmat, hg, geoms):
    """no surface point of the geoms lies more than 1 cm below the terrain under it (points beyond the terrain's edge: skipped)"""
    nrow, ncol, size, _ = hfield_ref.hfield_of(m, hg)
    worst = {}
    for i in range(gpos.shape[0]):
        Rh = gmat[i, hg].reshape(3, 3)
        for g in geoms:
            for pt in _surface_points(m, g, gpos[i, g], gmat[i, g].reshape(3, 3)):
                lp = Rh.T @ (pt - gpos[i, hg])
                if abs(lp[0]) > size[0] or abs(lp[1]) > size[1]:
                    continue
                d = pt[2] - _surface(m, hg, gpos[i, hg], gmat[i, hg], pt[:2])
                worst[g] = min(worst.get(g, 0.0), d)
    print("below the terrain, worst per geom (m):", {g: round(v, 4) for g, v in worst.items()})
    assert min(worst.values(), default=0.0) > -0.01, worst


@pytest.mark.parametrize("form", ["window", "fused", "many_body", "articulated"])
def test_every_form(lib, form):
    rng = np.random.default_rng(3)
    shapes = [(SPHERE, (0.07, 0, 0)), (BOX, (0.08, 0.06, 0.05)), (SPHERE, (0.05, 0, 0)), (CAPSULE, (0.05, 0.08, 0))]
    nrow, ncol = 24, 24
    elev = _terrain_elev(rng, nrow, ncol)
    try:
        if form == "fused":
            lib.mjh_set_window_solver(0)
        if form == "many_body":
            lib.mjh_set_layout_policy(2)
        m = _model(lib, elev, nrow, ncol, (1.2, 1.2, 0.12, 0.3), shapes=shapes, capacity=(64, 0), arm=form == "articulated")
        hg = m.name2id(2, "ground")
        nenv = 64
        e0 = ms.Engine(m, 1)
        gp0, gm0 = e0.get_geom_state(0, 1)
        if form == "window":
            assert e0.window_solver() == 1
        e0.close()
        buf = C.create_string_buffer(1 << 16)
        assert lib.mjh_debug_lds_layout(m.ptr, buf, len(buf)) >= 0
        if form == "many_body":
            assert "\nbig 1\n" in buf.value.decode()      # policy 2: the many-body layout
        q = np.tile(m.array("qpos0"), (nenv, 1))
        for i in range(nenv):
            for k in range(len(shapes)):
                xy = rng.uniform(-0.7, 0.7, size=2)
                q[i, 7 * k:7 * k + 3] = (xy[0], xy[1], _surface(m, hg, gp0[0, hg], gm0[0, hg], xy) + 0.1 + 0.1 * k)
        a = _run_form(m, nenv, q, 300, 1)
        b = _run_form(m, nenv, q, 300, 3)
        if form == "articulated":      # the arm's tip rests on the terrain
            e = ms.Engine(m, nenv)
            e.set_initial_qpos(q); e.reset(); e.step(300); e.synchronize()
            tip = m.name2id(2, "tip")
            touching = sum(any(g[0] == hg and g[1] == tip for g in e.get_contacts(i)["geom"]) for i in range(0, nenv, 4))
            e.close()
            assert touching >= nenv // 8, touching
    finally:
        lib.mjh_set_window_solver(1)
        lib.mjh_set_layout_policy(0)
    qq, vv, st, gpos, gmat = a
    assert np.isfinite(qq).all() and np.isfinite(vv).all()
    assert (st[:, 3] & 1).sum() == 0 and st[:, 0].max() > 0
    _check_above(m, gpos, gmat, hg, [g for g in range(m.ngeom) if g != hg])
    np.testing.assert_array_equal(a[0], b[0])
    np.testing.assert_array_equal(a[1], b[1])


def test_capacity_cap_and_flag(lib):
    """a tilted box over ~100 cells of a gently random terrain: the device keeps exactly the reference's first 50 contacts, in
    order (positions compared, so that another 50, another order or a shifted window would show); with a capacity of 30 the
    env's capacity flag is raised and the first 30 of them are kept whole"""
    nrow = ncol = 30
    cell = 2.0 / (ncol - 1)
    rng = np.random.default_rng(9)
    elev = (np.linspace(0, 1, ncol)[None, :] * 0.6 + 0.4 * rng.uniform(size=(nrow, ncol))).ravel()
    shapes = [(BOX, (0.35, 0.35, 0.05))]
    tilt = np.array(_qmul(_quat_z(0.3), (np.cos(0.01), np.sin(0.01), 0, 0)))
    out = {}
    for cap in (None, (30, 0)):
        m = _model(lib, elev, nrow, ncol, (1.0, 1.0, 0.03, 0.3), shapes=shapes, capacity=cap)
        hg, bx = m.name2id(2, "ground"), m.name2id(2, "g0")
        q = m.array("qpos0").copy(); q[0:3] = (0.03, -0.02, 0.015 + 0.05 - 0.006); q[3:7] = tilt
        e = ms.Engine(m, 2)
        e.set_initial_qpos(np.tile(q, (2, 1))); e.reset(); e.forward(); e.synchronize()
        gpos, gmat = e.get_geom_state()
        c = e.get_contacts(0)
        ref = hfield_ref.expected_contacts(m, hg, bx, gpos[0], gmat[0])
        full = hfield_ref.expected_contacts(m, hg, bx, gpos[0], gmat[0], maxcon=10 ** 6)
        assert len(full) > 60 and len(ref) == 50
        e.step(1); e.synchronize()
        out[cap] = (c, ref, e.get_stats()[:, 3].copy())
        e.close()
    c, ref, fl = out[None]
    assert len(c["dist"]) == 50 and (fl & 1).sum() == 0
    # the reference's prisms are all different places: each device contact lies where the reference's contact of the same rank does
    rp = np.array([x["pos"] for x in ref])
    nearest = [int(np.argmin(np.linalg.norm(rp[:, :2] - p[:2], axis=1))) for p in c["pos"]]
    assert nearest == list(range(50)), nearest
    np.testing.assert_allclose(c["dist"], [x["dist"] for x in ref], atol=3e-4)
    np.testing.assert_allclose(c["pos"][:, :2], rp[:, :2], atol=0.1 * cell)
    np.testing.assert_allclose(c["frame"][:, :3], [x["normal"] for x in ref], atol=0.05)
    c30, _, fl30 = out[(30, 0)]
    assert len(c30["dist"]) == 30 and (fl30 & 1).all()
    np.testing.assert_array_equal(c30["dist"], c["dist"][:30])
    np.testing.assert_array_equal(c30["pos"], c["pos"][:30])
    np.testing.assert_array_equal(c30["frame"], c["frame"][:30])
    np.testing.assert_allclose(c30["pos"][:, :2], rp[:30, :2], atol=0.1 * cell)


def test_soak(lib):
    rng = np.random.default_rng(11)
    shapes = [(SPHERE, (0.07, 0, 0)), (BOX, (0.08, 0.06, 0.05)), (SPHERE, (0.05, 0, 0)), (CYLINDER, (0.06, 0.05, 0))]
    nrow, ncol = 32, 32
    m = _model(lib, _terrain_elev(rng, nrow, ncol), nrow, ncol, (1.5, 1.5, 0.15, 0.3), shapes=shapes, capacity=(64, 0))
    hg = m.name2id(2, "ground")
    nenv = 4096
    e = ms.Engine(m, nenv)
    gp0, gm0 = e.get_geom_state(0, 1)
    q = np.tile(m.array("qpos0"), (nenv, 1))
    for i in range(nenv):
        for k in range(len(shapes)):
            xy = rng.uniform(-1.0, 1.0, size=2)
            q[i, 7 * k:7 * k + 3] = (xy[0], xy[1], _surface(m, hg, gp0[0, hg], gm0[0, hg], xy) + 0.15 + 0.12 * k)
    e.set_initial_qpos(q); e.reset(); e.step(1000); e.synchronize()
    t, qq, vv, _ = e.get_state()
    st = e.get_stats()
    gpos, gmat = e.get_geom_state()
    e.close()
    assert np.isfinite(qq).all() and np.isfinite(vv).all()
    assert (st[:, 3] & 1).sum() == 0
    assert np.allclose(t, 1000 * 0.002)          # no env was reset on the way
    _check_above(m, gpos[::16], gmat[::16], hg, [g for g in range(m.ngeom) if g != hg])
