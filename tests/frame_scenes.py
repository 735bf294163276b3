"""Models and states of the frame-state tests (tests/test_frame_ref.py on the CPU, tests/test_gpu_frame.py on the GPU), built through the
builder API.  Test infrastructure only.

rig(): a root body carrying THREE joints (slide x, slide y, hinge z: the odom pattern); under it a hinge chain of 4 bodies with
non-axis-aligned jnt_axis, non-zero jnt_pos and rotated body_quat; a BALL joint on a side link (with a hinge link behind it, so that the
ball's columns act on a descendant); a FREE body; a MOCAP body; sites with non-zero site_pos and rotated site_quat on the root, the chain's
tip, the ball branch, the free body and the mocap body.  Optionally a floor the moving bodies' spheres collide with.

chain(sizes): hinge / slide chains, one tree per entry of `sizes`, every body one joint (two hinges, then a slide, and so on) with random
unit axes, anchors and frames, no contacts.  The chains are compact — links of 2 cm, anchors within 1 cm, roots at the origin — and the FIRST
joint of a chain sits at its body's origin (the MJCF default).  The twist scale of the GPU test, sum |col| |qvel| per component, has no term
for the rounding of the levers p - anchor, 2^-23 |p|: where a body's few levers are much shorter than its coordinates, or one component of
axis x lever nearly cancels, that scale is far below the rounding of its inputs (measured on the one-hinge first bodies with an anchor 1 cm
off the body origin: ratio 667 with the roots 0.7 m from the origin, 98 with the roots at it, at absolute errors below 1e-6).
chain((70,)) is ONE chain of 70 dofs (the CPU reference test takes it); the engine refuses a tree of more than 64 dofs in a model of
more than 64 (mjh_create: MJH_ERR_CAPACITY, every constraint row maps one dof per lane), so the GPU tests take chain((6, 64)):
nv = 70 > 64, and the long chain's dofs 6 .. 69 lie on BOTH passes of the kernel's stride loop."""
import numpy as np

import mujoco_sim_amd as ms
from helpers import D, set_opt

GEOM_PLANE, GEOM_SPHERE = 0, 2
JNT_FREE, JNT_BALL, JNT_SLIDE, JNT_HINGE = 0, 1, 2, 3


def _unit(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def _ball_geom(lib, b, name, body, r, collide):
    lib.mjh_builder_add_geom(b, name, body, GEOM_SPHERE, D(r, 0, 0), None, None, None, -1, 1 if collide else 0, 0, -1)


def rig(lib, floor=False):
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002)
    if floor:
        lib.mjh_builder_add_geom(b, b"floor", 0, GEOM_PLANE, D(0, 0, 0.05), None, None, None, -1, 0, 1, -1)
    root = lib.mjh_builder_add_body(b, b"root", 0, D(0.1, -0.2, 0.8), D(*_unit([0.9, 0.1, -0.2, 0.3])), 0.0)
    lib.mjh_builder_add_joint(b, b"odom_x", root, JNT_SLIDE, D(0, 0, 0), D(1, 0, 0), None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_joint(b, b"odom_y", root, JNT_SLIDE, D(0, 0, 0), D(0, 1, 0), None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_joint(b, b"odom_yaw", root, JNT_HINGE, D(0.03, -0.02, 0.01), D(0, 0, 1), None, 0, 0, 0, 0, 0)
    _ball_geom(lib, b, b"g_root", root, 0.06, floor)
    rng = np.random.default_rng(3)
    parent, links = root, []
    for k in range(4):
        l = lib.mjh_builder_add_body(b, b"l%d" % (k + 1), parent, D(*rng.uniform(-0.15, 0.15, 3)), D(*_unit(rng.normal(size=4))), 0.0)
        lib.mjh_builder_add_joint(b, b"h%d" % (k + 1), l, JNT_HINGE, D(*rng.uniform(-0.05, 0.05, 3)), D(*_unit(rng.normal(size=3))), None, 0, 0, 0, 0, 0)
        _ball_geom(lib, b, b"g_l%d" % (k + 1), l, 0.04, floor)
        links.append(l); parent = l
    bl = lib.mjh_builder_add_body(b, b"bl", links[1], D(0.05, 0.1, -0.04), D(*_unit([0.7, -0.3, 0.5, 0.2])), 0.0)
    lib.mjh_builder_add_joint(b, b"ball", bl, JNT_BALL, D(0.02, -0.03, 0.01), None, None, 0, 0, 0, 0, 0)
    _ball_geom(lib, b, b"g_bl", bl, 0.04, floor)
    bl2 = lib.mjh_builder_add_body(b, b"bl2", bl, D(-0.06, 0.02, 0.09), D(*_unit([0.8, 0.2, 0.1, -0.4])), 0.0)
    lib.mjh_builder_add_joint(b, b"hb", bl2, JNT_HINGE, D(0.01, 0.02, -0.02), D(*_unit([0.3, -0.8, 0.5])), None, 0, 0, 0, 0, 0)
    _ball_geom(lib, b, b"g_bl2", bl2, 0.03, floor)
    fb = lib.mjh_builder_add_body(b, b"fb", 0, D(0.7, 0.4, 0.6), None, 0.0)
    lib.mjh_builder_add_joint(b, b"fb_free", fb, JNT_FREE, None, None, None, 0, 0, 0, 0, 0)
    _ball_geom(lib, b, b"g_fb", fb, 0.05, floor)
    mc = lib.mjh_builder_add_body(b, b"mc", 0, D(-0.5, 0.3, 0.4), D(*_unit([0.6, 0.4, -0.5, 0.3])), 0.0)
    lib.mjh_builder_set_mocap(b, mc)
    lib.mjh_builder_add_site(b, b"s_root", root, D(0.05, -0.02, 0.1), D(*_unit([0.9, 0.1, -0.3, 0.2])))
    lib.mjh_builder_add_site(b, b"s_tip", links[3], D(0.02, 0.07, -0.11), D(*_unit([0.5, -0.5, 0.4, 0.6])))
    lib.mjh_builder_add_site(b, b"s_ball", bl2, D(-0.03, 0.04, 0.05), D(*_unit([0.3, 0.8, -0.2, 0.4])))
    lib.mjh_builder_add_site(b, b"s_free", fb, D(0.04, 0.03, -0.06), D(*_unit([0.7, 0.2, 0.6, -0.3])))
    lib.mjh_builder_add_site(b, b"s_mocap", mc, D(0.1, -0.05, 0.02), D(*_unit([0.4, -0.6, 0.3, 0.6])))
    m = ms.Model(lib.mjh_builder_compile(b), lib); lib.mjh_builder_destroy(b)
    return m


def chain(lib, sizes=(6, 64), seed=9):
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002)
    rng = np.random.default_rng(seed)
    for t, size in enumerate(sizes):
        parent = 0
        for k in range(size):
            pos = rng.uniform(-1, 1, 3) * 0.02
            l = lib.mjh_builder_add_body(b, b"c%d_%d" % (t, k), parent, D(*pos), D(*_unit(rng.normal(size=4))), 0.0)
            jpos = rng.uniform(-0.01, 0.01, 3) * (0.0 if k == 0 else 1.0)
            lib.mjh_builder_add_joint(b, b"j%d_%d" % (t, k), l, JNT_SLIDE if k % 3 == 2 else JNT_HINGE, D(*jpos), D(*_unit(rng.normal(size=3))), None, 0, 0, 0, 0, 0)
            _ball_geom(lib, b, b"g%d_%d" % (t, k), l, 0.01, False)
            if k in (size // 2, size - 1):
                lib.mjh_builder_add_site(b, b"s%d_%d" % (t, k), l, D(*rng.uniform(-0.03, 0.03, 3)), D(*_unit(rng.normal(size=4))))
            parent = l
    m = ms.Model(lib.mjh_builder_compile(b), lib); lib.mjh_builder_destroy(b)
    return m


def states(m, nenv, seed=21, slide=0.05):
    """qpos [nenv, nq] (random angles, slides within +-slide of qpos0, unit quaternions, free positions near qpos0), qvel [nenv, nv] in
    [-2, 2], mocap [nenv, nmocap, 7] (pos, unit quat), all different per env"""
    from indep_dyn import Tree
    tr = Tree(m)
    rng = np.random.default_rng(seed)
    q = np.zeros((nenv, m.nq)); v = rng.uniform(-2, 2, (nenv, m.nv)); mocap = np.zeros((nenv, m.nmocap, 7))
    for i in range(nenv):
        q[i] = tr.q0
        for j in range(tr.nj):
            a, t = tr.jq[j], tr.jtype[j]
            if t == JNT_FREE:
                q[i, a:a + 3] += rng.uniform(-0.5, 0.5, 3); q[i, a + 3:a + 7] = _unit(rng.normal(size=4))
            elif t == JNT_BALL:
                q[i, a:a + 4] = _unit(rng.normal(size=4))
            elif t == JNT_SLIDE:
                q[i, a] += rng.uniform(-slide, slide)
            else:
                q[i, a] += rng.uniform(-np.pi, np.pi)
        for k in range(m.nmocap):
            mocap[i, k, :3] = rng.uniform(-1, 1, 3); mocap[i, k, 3:] = _unit(rng.normal(size=4))
    return q, v, mocap
