"""Scenes of the contact-report tests (CPU reference test and GPU tests), each the smallest that reaches its code, with per-env jittered
poses in clear penetration (every contact at least 1e-4 inside the activation margin of 0: tests/test_contact_ref.py checks it on the
oracle).  Test infrastructure only."""
import numpy as np

import mujoco_sim_amd as ms
from helpers import D, set_opt

PEN = 0.003      # penetration of every resting contact [m]
GEOM_PLANE, GEOM_SPHERE, GEOM_CAPSULE, GEOM_BOX = 0, 2, 3, 6
JNT_FREE, JNT_SLIDE, JNT_HINGE = 0, 2, 3


def _free(lib, b, name, pos):
    bd = lib.mjh_builder_add_body(b, name, 0, D(*pos), None, 0.0)
    lib.mjh_builder_add_joint(b, name + b"_free", bd, JNT_FREE, None, None, None, 0, 0, 0, 0, 0)
    return bd


def _yaw(a):
    return np.array([np.cos(a / 2), 0.0, 0.0, np.sin(a / 2)])


# ------------------------------------------------------------------ scene 1: free bodies
def free_scene(lib, condim=3, noslip=0, maxcon=None):
    """floor, box A on it, smaller box B (yawed) on A, a sphere on the floor: 4 + 4 + 1 contacts"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002, noslip_iterations=noslip)
    lib.mjh_builder_add_geom(b, b"floor", 0, GEOM_PLANE, D(0, 0, 0.05), None, None, None, condim, -1, -1, -1)
    A = _free(lib, b, b"A", (0, 0, 0.1))
    lib.mjh_builder_add_geom(b, b"gA", A, GEOM_BOX, D(0.15, 0.15, 0.1), None, None, None, condim, -1, -1, -1)
    B = _free(lib, b, b"B", (0, 0, 0.25))
    lib.mjh_builder_add_geom(b, b"gB", B, GEOM_BOX, D(0.05, 0.05, 0.05), None, None, None, condim, -1, -1, -1)
    S = _free(lib, b, b"S", (0.5, 0, 0.08))
    lib.mjh_builder_add_geom(b, b"gS", S, GEOM_SPHERE, D(0.08, 0, 0), None, None, None, condim, -1, -1, -1)
    if maxcon is not None:
        lib.mjh_builder_set_capacity(b, maxcon, 4 * 16 + 8)
    m = ms.Model(lib.mjh_builder_compile(b), lib); lib.mjh_builder_destroy(b)
    return m


FREE_NCON = 9


def free_states(m, nenv, seed=11, spin=0.0):
    """qpos [nenv, nq], qvel [nenv, nv]: the stack with per-env offsets and yaws; spin: angular velocity of the sphere about z"""
    rng = np.random.default_rng(seed)
    q = np.zeros((nenv, m.nq)); v = np.zeros((nenv, m.nv))
    for i in range(nenv):
        ax, ay = rng.uniform(-0.02, 0.02, 2); ya = rng.uniform(-0.05, 0.05)
        bx, by = rng.uniform(-0.02, 0.02, 2); yb = 0.4 + rng.uniform(-0.05, 0.05)
        sx, sy = rng.uniform(-0.02, 0.02, 2)
        q[i, 0:7] = [ax, ay, 0.1 - PEN, *_yaw(ya)]
        q[i, 7:14] = [ax + bx, ay + by, 0.2 - PEN + 0.05 - PEN, *_yaw(yb)]
        q[i, 14:21] = [0.5 + sx, sy, 0.08 - PEN, 1, 0, 0, 0]
        v[i, 17] = spin
    return q, v


# ------------------------------------------------------------------ scene 2: articulated
L1 = L2 = 0.3
RCAP = 0.04
HBOX = 0.06


def arm_scene(lib, sensor=False):
    """a slide + two-hinge arm whose capsule tip presses the floor, a free box on the floor with one vertical edge pressed into the arm's
    second link, a free ball connected to the arm's base, a free cube welded (torquescale 0.9) to the world; optionally a force sensor on
    the second link (the oracle then fills its own cfrc_ext)"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002)
    lib.mjh_builder_add_geom(b, b"floor", 0, GEOM_PLANE, D(0, 0, 0.05), None, None, None, -1, -1, -1, -1)
    base = lib.mjh_builder_add_body(b, b"base", 0, D(0, 0, 0.6), None, 0.0)
    lib.mjh_builder_add_joint(b, b"slide", base, JNT_SLIDE, None, D(0, 0, 1), None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"gbase", base, GEOM_SPHERE, D(0.05, 0, 0), D(0, 0, 0.1), None, None, -1, -1, -1, -1)
    l1 = lib.mjh_builder_add_body(b, b"l1", base, D(0, 0, 0), None, 0.0)
    lib.mjh_builder_add_joint(b, b"h1", l1, JNT_HINGE, D(0, 0, 0), D(0, 1, 0), None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"g1", l1, GEOM_CAPSULE, D(RCAP, L1 / 2, 0), D(0, 0, -L1 / 2), None, None, -1, -1, -1, -1)
    l2 = lib.mjh_builder_add_body(b, b"l2", l1, D(0, 0, -L1), None, 0.0)
    lib.mjh_builder_add_joint(b, b"h2", l2, JNT_HINGE, D(0, 0, 0), D(0, 1, 0), None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"g2", l2, GEOM_CAPSULE, D(RCAP, L2 / 2, 0), D(0, 0, -L2 / 2), None, None, -1, -1, -1, -1)
    if sensor:
        s = lib.mjh_builder_add_site(b, b"s2", l2, D(0.01, 0.0, -0.1), D(0.9, 0.1, -0.3, 0.2))
        lib.mjh_builder_add_sensor(b, b"f2", 4, s)
    box = _free(lib, b, b"box", (0.3, 0.3, HBOX))
    lib.mjh_builder_add_geom(b, b"gbox", box, GEOM_BOX, D(HBOX, HBOX, HBOX), None, None, None, -1, -1, -1, -1)
    bob = _free(lib, b, b"bob", (0.4, 0.5, 0.9))
    lib.mjh_builder_add_geom(b, b"gbob", bob, GEOM_SPHERE, D(0.05, 0, 0), None, None, None, -1, -1, -1, -1)
    lib.mjh_builder_add_eq_connect(b, bob, base, D(0.0, -0.2, 0.0))
    cube = _free(lib, b, b"cube", (1.0, 0, 0.6))
    lib.mjh_builder_add_geom(b, b"gcube", cube, GEOM_BOX, D(0.05, 0.05, 0.05), None, None, None, -1, -1, -1, -1)
    lib.mjh_builder_add_eq_weld(b, cube, 0, None, 0.9)
    lib.mjh_builder_set_capacity(b, 16, 16 * 4 + 12)
    m = ms.Model(lib.mjh_builder_compile(b), lib); lib.mjh_builder_destroy(b)
    return m


ARM_NCON = 6      # tip-floor 1, box-floor 4, box-arm 1


def arm_states(m, nenv, seed=5):
    """qpos [nenv, nq], qvel, xfrc_applied [nenv, nbody, 6]: joint order slide, h1, h2, box, bob, cube"""
    rng = np.random.default_rng(seed)
    q = np.zeros((nenv, m.nq)); v = np.zeros((nenv, m.nv)); xf = np.zeros((nenv, m.nbody, 6))
    l2, bob = m.name2id(0, "l2"), m.name2id(0, "bob")
    for i in range(nenv):
        q1 = 0.4 + rng.uniform(-0.03, 0.03); q2 = -0.9 + rng.uniform(-0.03, 0.03)
        d1 = np.array([-np.sin(q1), 0.0, -np.cos(q1)]); d2 = np.array([-np.sin(q1 + q2), 0.0, -np.cos(q1 + q2)])
        # base height: the tip sphere's lowest point PEN below the floor
        zb = RCAP - PEN - (L1 * d1[2] + L2 * d2[2])
        elbow = np.array([0.0, 0.0, zb]) + L1 * d1
        # the box: on the floor, yawed, its lowest-y vertical edge PEN inside the second link's cylinder at 80 % of its length
        t = 0.8 + rng.uniform(-0.03, 0.03)
        xe = (elbow + t * L2 * d2)[0]; ye = RCAP - PEN
        psi = 0.5 + rng.uniform(-0.05, 0.05)
        c, s = np.cos(psi), np.sin(psi)
        ctr = np.array([xe, ye]) + np.array([c * HBOX - s * HBOX, s * HBOX + c * HBOX])
        q[i, 0:3] = [zb - 0.6, q1, q2]
        q[i, 3:10] = [ctr[0], ctr[1], HBOX - PEN, *_yaw(psi)]
        q[i, 10:17] = [0.4 + rng.uniform(-0.01, 0.01), 0.5 + rng.uniform(-0.01, 0.01), 0.9 + zb - 0.6 + rng.uniform(-0.01, 0.01), 1, 0, 0, 0]
        cq = np.array([1.0, *rng.uniform(-0.02, 0.02, 3)]); cq /= np.linalg.norm(cq)
        q[i, 17:24] = [1.0 + rng.uniform(-0.005, 0.005), rng.uniform(-0.005, 0.005), 0.6 + rng.uniform(-0.005, 0.005), *cq]
        xf[i, l2] = [1.0, 2.0, -3.0, 0.1, -0.2, 0.05] + rng.uniform(-0.1, 0.1, 6)
        xf[i, bob, :3] = rng.uniform(-1, 1, 3)
    return q, v, xf


def oracle_at(m, q, v, xf=None):
    """one oracle env teacher-forced to (q, v), zero warm start"""
    import orc
    d = orc.OrcData(m.ptr)
    d.set_qpos(q); d.call("reset")
    d.f("qvel")[:] = v
    if xf is not None:
        d.f("xfrc_applied")[:] = np.asarray(xf).reshape(-1)
    return d
