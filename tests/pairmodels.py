"""Models, cases and bookkeeping shared by the tests of the analytic pairs (tests/test_pairgeom.py: oracle; tests/test_collide_host.py:
the device's routines on the host; tests/test_gpu_pairs.py: device): one small model per pair type — a static plane (horizontal, or
tilted) or one free body, plus one free body — whose envs get their own pose and geom sizes, the families of tests/pairgeom.py posed
for such a model, the oracle's contacts of a case, and the per-family summary line.  Test infrastructure only."""
import ctypes as C

import numpy as np
import mujoco_sim_amd as ms
import orc
import pairgeom as pg
from helpers import D, set_opt
from mujoco_sim_amd.engine import EP

LADDER = [1e-9 * 10 ** (k / 2) for k in range(15)]      # half decades from 1e-9
CAP = 0.02
PLANES = [(np.array([1.0, 0, 0, 0]), np.zeros(3)),
          (pg.rot_quat([0.8, -0.5, 0.2], 0.9), np.array([0.1, -0.05, 0.08]))]      # horizontal; a normal that is not z


def mesh_cloud():
    """16 points on a lumpy ellipsoid: all of them hull vertices"""
    rng = np.random.default_rng(77)
    v = rng.normal(size=(16, 3)); v /= np.linalg.norm(v, axis=1)[:, None]
    return v * np.array([0.09, 0.07, 0.05]) * rng.uniform(0.85, 1.0, size=(16, 1))


def pair_model(lib, family, plane=None):
    """(model, g1, g2): the family's two geoms; a plane family's plane is static at `plane` = (quat, pos)"""
    t1, t2 = (pg.TYPES[x] for x in family.split("_"))
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.005)
    default = {pg.SPHERE: (0.05, 0, 0), pg.CAPSULE: (0.05, 0.1, 0), pg.CYLINDER: (0.05, 0.1, 0), pg.ELLIPSOID: (0.1, 0.05, 0.03), pg.BOX: (0.1, 0.08, 0.06)}

    def free(name, t, z):
        bd = lib.mjh_builder_add_body(b, name, 0, D(0, 0, z), None, 0.0)
        lib.mjh_builder_add_joint(b, None, bd, 0, None, None, None, 0, 0, 0, 0, 0)
        if t == pg.MESH:
            v = np.ascontiguousarray(mesh_cloud())
            mid = lib.mjh_builder_add_mesh(b, v.ctypes.data_as(C.POINTER(C.c_double)), len(v), None, 0, None)
            assert mid == 0, lib.mjh_last_error()
            assert lib.mjh_builder_add_mesh_geom(b, None, bd, mid, None, None, None, -1, -1, -1, 1000.0) >= 0
        else:
            lib.mjh_builder_add_geom(b, None, bd, t, D(*default[t]), None, None, None, -1, -1, -1, -1)
    if t1 == pg.PLANE:
        lib.mjh_builder_add_geom(b, b"plane", 0, 0, D(0, 0, 0.05), D(*plane[1]), D(*plane[0]), None, -1, -1, -1, -1)
    else:
        free(b"a", t1, 1.0)
    free(b"b", t2, 2.0)
    m = ms.Model(lib.mjh_builder_compile(b), lib)
    lib.mjh_builder_destroy(b)
    assert m.ngeom == 2 and m.npair == 1 and list(m.array("geom_type")) == [t1, t2]
    return m


class Family:
    """the cases of a family and what a model needs to pose them: qpos and the per-env geom sizes / bounding radii"""

    def __init__(self, lib, family, n, seed, plane=None):
        self.name, self.plane = family, plane
        self.m = m = pair_model(lib, family, plane)
        self.t = [int(x) for x in m.array("geom_type")]
        self.mesh = m.array("mesh_vert").reshape(-1, 3).copy() if self.t[1] == pg.MESH else None
        self.lpos, self.lquat = m.array("geom_pos").reshape(-1, 3).copy(), m.array("geom_quat").reshape(-1, 4).copy()
        self.cases = pg.cases(family, n, seed, plane=plane, mesh=self.mesh)
        self.qpos = np.array([self._qpos(c) for c in self.cases])
        self.size = np.tile(m.array("geom_size"), (n, 1)).reshape(n, 2, 3)
        self.rbound = np.tile(m.array("geom_rbound"), (n, 1))
        for i, c in enumerate(self.cases):
            for k, g in enumerate((c["g1"], c["g2"])):
                if g[0] not in (pg.PLANE, pg.MESH):
                    self.size[i, k] = g[3][:3]
                    self.rbound[i, k] = lib_rbound(g[0], g[3])

    def _qpos(self, c):
        out = []
        for k, (g, q) in enumerate(((c["g1"], c["q1"]), (c["g2"], c["q2"]))):
            if g[0] == pg.PLANE:
                continue
            ql = self.lquat[k]
            qb = pg.quat_mul(q, ql * np.array([1, -1, -1, -1]))          # geom pose = body pose o local pose
            out += list(g[1] - pg.quat_mat(qb) @ self.lpos[k]) + list(qb)
        return out

    def geoms(self, gpos, gmat, i):
        """the reference geoms of case i from exported geom poses"""
        return tuple((self.t[k], np.asarray(gpos[k], float), np.asarray(gmat[k], float).reshape(3, 3),
                      self.mesh if self.t[k] == pg.MESH else self.size[i, k].copy()) for k in range(2))


def lib_rbound(t, s):
    return {pg.SPHERE: s[0], pg.CAPSULE: s[0] + s[1], pg.CYLINDER: np.hypot(s[0], s[1]), pg.BOX: np.linalg.norm(s[:3]), pg.ELLIPSOID: max(s[:3])}[t]


_families = {}


def families(lib, family, n, seed=20261018):
    """a family's cases over its models: one for a round pair, one per plane pose for a plane pair (built once per session)"""
    key = (family, n, seed)
    if key not in _families:
        if family.startswith("plane_"):
            _families[key] = [Family(lib, family, n // len(PLANES), seed + k, plane=p) for k, p in enumerate(PLANES)]
        else:
            _families[key] = [Family(lib, family, n, seed)]
    return _families[key]


def oracle_contacts(fam, d, i):
    d.set_env_param(EP["geom_size"], fam.size[i]); d.set_env_param(EP["geom_rbound"], fam.rbound[i])
    d.set_qpos(fam.qpos[i]); d.call("kinematics"); d.call("collision")
    g1, g2 = fam.geoms(d.f("geom_xpos").reshape(-1, 3), d.f("geom_xmat").reshape(-1, 9), i)
    c = d.contacts()
    return g1, g2, np.array([x["dist"] for x in c]), np.array([x["pos"] for x in c]).reshape(-1, 3), np.array([x["frame"][:3] for x in c]).reshape(-1, 3)


def needed_tol(g1, g2, dist, pos, n, ladder=LADDER, margin=0.0, D=None):
    """the smallest tolerance of the ladder at which the contact list passes (inf: none)"""
    for tol in ladder:
        if not pg.check_contacts(g1, g2, margin, dist, pos, n, tol=tol, D=D):
            return tol
    return np.inf


def summarize(name, rows, tol):
    """rows: (robust, touching, violations, needed tolerance, tag).  Prints the family's figures, returns the failures"""
    nrob = sum(r[0] for r in rows); ntouch = sum(r[0] and r[1] for r in rows)
    fails = [(i, r[4], r[2][:3]) for i, r in enumerate(rows) if r[0] and r[2]]
    worst = max([r[3] for r in rows if r[0]], default=0.0)
    print(f"PAIRGEOM {name}: {len(rows)} cases, non-robust {1 - nrob / len(rows):.4f}, robust touching {ntouch}, "
          f"violations at {tol:g}: {len(fails)}, passes from {worst:.1e}")
    return nrob, ntouch, fails, worst


