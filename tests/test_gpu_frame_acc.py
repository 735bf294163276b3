"""Frame accelerations on the device (mjh_frame_accel / mjh_frame_accel_device, csrc/frame_acc.hip) against the numpy fp64 reference of
tests/frame_acc_ref.py, evaluated at the device's OWN fp32 state (qpos and qvel read back by get_state, qacc by get_field; mocap poses
rounded to fp32).  qacc is set through set_state(warmstart=...) with random values, so only the frame arithmetic is under test, not the
stepper.  Models and states: tests/frame_scenes.py, 5 envs with different states.

Parity bound:  err <= C 2^-23 depth s,  depth = bodies in the frame's chain, s per component from the reference: the sum of the absolute
values of every elementary product that enters it (|J| |qacc|, the pairwise terms of Jdot qvel, |gravity| with PROPER; through |R^T| with
LOCAL).  A component with s = 0 is exactly zero.  C is four times the worst ratio measured on the MI355X over the cases here, rounded up
to a power of two (the margin is for other seeds), as tests/test_gpu_frame.py derived its 64.
Measured worst err / (2^-23 depth s), acceleration / bias:
    rig (17 dofs: odom joints, hinges, ball, free, mocap)      3.51 / 3.23
    rig with a floor, after three steps                        24.03 / 1.37
    chains of 6 and 64 dofs (nv = 70)                          26.81 / 2.39
so C = 128 (4 x 26.81 = 107, rounded up): above the twist's 64.  The excess is in the direct part J qacc (the bias alone stays below 4), whose
columns are the twist's.  The lever roundings p - anchor (tests/frame_scenes.py) were the candidate and are NOT the cause here: with the
size of the levers' inputs (`lever` of tests/frame_acc_ref.py) added to the scale the same ratios read 3.51 / 24.03 / 26.45, measured.
Nor is the absolute rounding of the unit axes (`axis` there): 3.51 / 24.03 / 26.81 with it added, measured.  The parity test prints the
place of its worst case, and on all three models it is a LOCAL | PROPER frame of depth 1, z component, whose value is the single term
R[2][2] |g| with a small R[2][2] (0.649 = 0.066 |g| on the chain, err 2.07e-06 = 1.8 x 2^-23 |g|): the entries of the frame's rotation
matrix are sums of quaternion products that cancel, so they carry an ABSOLUTE error near 2^-23, and the scale |R^T| s rates a small
entry's term by the entry's size.  That reading of the worst cases is an inference from their place and size, not a separate measurement.
Independently of C every component also satisfies the ray rule |err| <= 5e-5 max(1, s) (tests/ray_check.py).

Identities on the device's own output are held to summation rounding, derived in place."""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
from mujoco_sim_amd import capi
import frame_ref as fr
import frame_acc_ref as far
import frame_scenes as fs
import ray_check
from helpers import D, set_opt

pytestmark = pytest.mark.gpu
NENV = 5
EPS = 2.0 ** -23
C_BOUND = 128.0
RAY_TOL = ray_check.TOL
FLAGS = [{}, dict(local=True), dict(proper=True), dict(local=True, proper=True)]


# ------------------------------------------------------------------ models, states, engines and frame lists: made once, never changed
_CACHE = {}


@pytest.fixture(scope="module", autouse=True)
def _engines_are_closed():
    """the cached engines are closed when the module's last test has run"""
    yield
    for c in _CACHE.values():
        c["e"].close()
    _CACHE.clear()


def _every_frame(m):
    """every body (the world and the mocap body included) and site: plain, LOCAL, PROPER and LOCAL | PROPER"""
    plain = [("body", b) for b in range(m.nbody)] + [("site", s) for s in range(m.nsite)]
    return [(t, i, opt) if opt else (t, i) for opt in FLAGS for (t, i) in plain]


def _set(e, m, q, v, qacc, mocap):
    e.set_state(qpos=q, qvel=v, time=np.zeros(len(q)), warmstart=qacc)
    for k in range(m.nmocap):
        e.set_mocap_pose(k, mocap[:, k, :3], mocap[:, k, 3:])


def _case(lib, name):
    if name in _CACHE:
        return _CACHE[name]
    if name == "rig":
        m = fs.rig(lib); q, v, mocap = fs.states(m, NENV, slide=0.5)
    else:
        m = fs.chain(lib, (6, 64)); q, v, mocap = fs.states(m, NENV)
        assert m.nv == 70 and list(m.array("tree_dofadr")) == [0, 6]      # the long chain's dofs lie on both passes of the stride loop
    qacc = np.random.default_rng(17).uniform(-5, 5, v.shape)
    e = ms.Engine(m, NENV)
    _set(e, m, q, v, qacc, mocap)
    _CACHE[name] = dict(m=m, e=e, R=far.FrameAccRef(m), frames=_every_frame(m), mocap=mocap.astype(np.float32).astype(np.float64))
    return _CACHE[name]


def _six(out, a, b):
    return np.concatenate([out[a], out[b]], axis=-1)


def _parity(name, c, e=None):
    """the device's accelerations and biases of every env against the reference at the device's own state; returns the worst ratios"""
    m, R, frames = c["m"], c["R"], c["frames"]
    e = e or c["e"]
    _, qd, vd, _ = e.get_state()
    ad = e.get_field("qacc")
    out = e.frame_accel(frames, bias=True)
    acc, bias = _six(out, "linacc", "angacc"), _six(out, "biasp", "biasr")
    tup = [far.accel_tuple(m, f) for f in frames]
    depth = np.array([R.depth(t, j) for (t, j, _) in tup], float)[:, None]
    worst = dict(acc=0.0, bias=0.0, ray=0.0, lever=0.0, axis=0.0)
    where = None
    for i in range(NENV):
        ref = R.evaluate_acc(qd[i], vd[i], ad[i], tup, c["mocap"][i])
        for key, dev, want, s in (("acc", acc[i], _six(ref, "linacc", "angacc"), ref["s"]), ("bias", bias[i], _six(ref, "biasp", "biasr"), ref["sb"])):
            err = np.abs(dev - want)
            assert (err[s == 0] == 0).all(), (name, key, i, np.argwhere((s == 0) & (err != 0)))      # no terms: exactly zero
            ratio = np.where(s > 0, err / (EPS * depth * np.where(s > 0, s, 1.0)), 0.0)
            if key == "acc" and ratio.max() > worst["acc"]:
                k, r = np.unravel_index(ratio.argmax(), ratio.shape)
                where = (i, frames[k], int(r), float(depth[k, 0]), float(s[k, r]), float(err[k, r]), float(want[k, r]))
            worst[key] = max(worst[key], ratio.max())
            worst["ray"] = max(worst["ray"], (err / np.maximum(1.0, s)).max())
            if key == "acc":      # a diagnostic, not a bound: the same ratio with the size of the levers' inputs added to the scale
                worst["lever"] = max(worst["lever"], np.where(s > 0, err / (EPS * depth * np.where(s > 0, s + ref["lever"], 1.0)), 0.0).max())
                worst["axis"] = max(worst["axis"], np.where(s > 0, err / (EPS * depth * np.where(s > 0, s + ref["axis"], 1.0)), 0.0).max())
    print(f"[{name}] worst err / (2^-23 depth s): acceleration {worst['acc']:.2f}, bias {worst['bias']:.2f}; "
          f"worst err / max(1, s): {worst['ray']:.2e} (ray rule {RAY_TOL:.0e}); C = {C_BOUND}; "
          f"acceleration with the levers' inputs in the scale: {worst['lever']:.2f}, with unit axes in the scale: {worst['axis']:.2f}; "
          f"worst acceleration at (env, frame, component, depth, s, err, value) {where}")
    assert worst["ray"] <= RAY_TOL, (name, worst)
    assert max(worst["acc"], worst["bias"]) <= C_BOUND, (name, worst)
    return worst


# ------------------------------------------------------------------ 1. parity with the reference
@pytest.mark.parametrize("name", ["rig", "chain"])
def test_parity_with_the_reference(name, lib):
    _parity(name, _case(lib, name))


# ------------------------------------------------------------------ 2. identities on the device's own output
@pytest.mark.parametrize("name", ["rig", "chain"])
def test_identities_on_the_devices_own_output(name, lib):
    c = _case(lib, name); m, e, R = c["m"], c["e"], c["R"]
    plain = [("body", b) for b in range(m.nbody)] + [("site", s) for s in range(m.nsite)]
    npl = len(plain)
    out = e.frame_accel(c["frames"], bias=True)
    acc, bias = _six(out, "linacc", "angacc"), _six(out, "biasp", "biasr")
    st = e.frame_state(plain, jacobian=True)
    ad = e.get_field("qacc")
    da, dn = m.array("body_dofadr"), m.array("body_dofnum")
    sb = m.array("site_bodyid")
    g32 = np.array([m.opt.gravity[k] for k in range(3)], dtype=np.float32)
    assert np.abs(g32).max() > 1
    worst = 0.0
    for i in range(NENV):
        for k, (t, j) in enumerate(plain):
            b = R.body_of(fr.SITE if t == "site" else fr.BODY, j)
            nchain = sum(int(dn[a]) for a in R.chain[b])
            # acc - bias = J qacc, formed in fp64 from the device's Jacobian and qacc.  On the device direct = sum_d c_d qacc_d carries one
            # rounding per product and up to nchain for the sums (lanes and butterfly), relative to sum |c_d qacc_d|; acc = fl(direct +
            # bias) adds half an ulp of |acc| <= sum |c_d qacc_d| + |bias|:  (nchain + 1) 2^-23 (|J| |qacc| + |bias|) covers both
            J = np.concatenate([st["jacp"][i, k], st["jacr"][i, k]])
            bound = (nchain + 1) * EPS * (np.abs(J) @ np.abs(ad[i]) + np.abs(bias[i, k]))
            err = np.abs(acc[i, k] - bias[i, k] - J @ ad[i])
            assert (err <= bound).all(), (name, i, t, j, err, bound)
            worst = max(worst, (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
            if t == "site":      # a site and its body: bitwise the same angular acceleration and angular bias
                assert np.array_equal(acc[i, k, 3:6], acc[i, sb[j], 3:6]) and np.array_equal(bias[i, k, 3:6], bias[i, sb[j], 3:6]), (name, i, j)
            for n in (1, 2, 3):      # the bias with LOCAL or PROPER set is bitwise the bias without
                assert np.array_equal(bias[i, n * npl + k], bias[i, k]), (name, i, t, j, n)
            # PROPER changes linacc by exactly fl(linacc - g), and nothing else
            lin32 = acc[i, k, 0:3].astype(np.float32)
            assert np.array_equal(acc[i, 2 * npl + k, 0:3], (lin32 - g32).astype(np.float64)), (name, i, t, j)
            assert np.array_equal(acc[i, 2 * npl + k, 3:6], acc[i, k, 3:6])
    print(f"[{name}] identity acc - bias = J qacc, worst error / bound: {worst:.2f}")
    stills = [0] + ([m.name2id(0, "mc"), m.nbody + m.name2id(3, "s_mocap")] if name == "rig" else [])
    for k in stills:      # the world, the mocap body and its site: zeros (and -g with PROPER, in world axes)
        assert not acc[:, k].any() and not bias[:, k].any() and not acc[:, npl + k].any() and not bias[:, 2 * npl + k].any()
        assert np.array_equal(acc[:, 2 * npl + k, 0:3], np.broadcast_to(-g32.astype(np.float64), (NENV, 3))) and not acc[:, 2 * npl + k, 3:6].any()


def test_a_unit_qacc_reads_the_jacobian_column_of_frame_state_bitwise(lib):
    """qvel = 0 and qacc = e_d: the bias has no term, the direct sum is the one product c_d * 1 among zeros, so acc is the column d the kernel
    staged and walked — which must be the bits of mjh_frame_state's Jacobian (frame_acc.hip writes frame.hip's stage and pose a second time)"""
    m = fs.rig(lib)
    q, _, mocap = fs.states(m, NENV, slide=0.5)
    jt, ja = [int(t) for t in m.array("jnt_type")], [int(a) for a in m.array("jnt_dofadr")]
    ball, free = ja[jt.index(fs.JNT_BALL)], ja[jt.index(fs.JNT_FREE)]
    # one dof per env: the second odom slide, the odom hinge behind the slides, a ball column, the hinge behind the ball, a free rotation
    dofs = [ja[jt.index(fs.JNT_SLIDE)] + 1, ja[jt.index(fs.JNT_HINGE)], ball + 1, ball + 3, free + 4]
    assert jt[m.array("dof_jntid")[ball + 3]] == fs.JNT_HINGE
    assert len(set(dofs)) == NENV and all(0 <= d < m.nv for d in dofs)
    qacc = np.zeros((NENV, m.nv))
    for i, d in enumerate(dofs):
        qacc[i, d] = 1.0
    e = ms.Engine(m, NENV)
    _set(e, m, q, np.zeros((NENV, m.nv)), qacc, mocap)
    plain = [("body", b) for b in range(m.nbody)] + [("site", s) for s in range(m.nsite)]
    out = e.frame_accel(plain, bias=True)
    st = e.frame_state(plain, jacobian=True)
    assert not out["biasp"].any() and not out["biasr"].any()
    seen = 0
    for i, d in enumerate(dofs):
        colp, colr = st["jacp"][i, :, :, d], st["jacr"][i, :, :, d]
        assert np.array_equal(out["linacc"][i], colp) and np.array_equal(out["angacc"][i], colr), (i, d)
        seen += int(np.count_nonzero(colp)) + int(np.count_nonzero(colr))
    assert seen > 50      # not vacuous: the columns have entries
    e.close()


# ------------------------------------------------------------------ 3. bitwise independence
def _bits(d):
    return np.concatenate([d[k] for k in ("linacc", "angacc")], axis=-1).view(np.int64)


def _bbits(d):
    return np.concatenate([d[k] for k in ("biasp", "biasr")], axis=-1).view(np.int64)


def _sbits(d):
    return np.concatenate([d[k] for k in ("pos", "quat", "linvel", "angvel")], axis=-1).view(np.int64)


@pytest.mark.parametrize("name", ["rig", "chain"])
def test_a_frame_does_not_depend_on_the_call_around_it(name, lib):
    import torch
    c = _case(lib, name); m, e = c["m"], c["e"]
    ns, nb = m.nsite, m.nbody
    LP = dict(local=True, proper=True)
    eight = [("site", ns - 1, LP), ("body", nb - 1, dict(local=True)), ("site", ns - 1), ("body", 1), ("site", 0, dict(proper=True)),
             ("body", nb // 2, LP), ("site", ns - 1, dict(local=True)), ("body", nb - 1)]
    with_bias = e.frame_accel(eight, bias=True)
    full, fullb = _bits(with_bias), _bbits(with_bias)
    assert np.array_equal(_bits(e.frame_accel(eight)), full)                                 # without the bias output
    sub = e.frame_accel(eight, env0=3, n=1, bias=True)                                       # another range
    assert np.array_equal(_bits(sub)[0], full[3]) and np.array_equal(_bbits(sub)[0], fullb[3])
    assert np.array_equal(_bits(e.frame_accel(eight, env0=1, n=3))[2], full[3])
    for k in (0, 2, 5):                                                                      # alone in a call, with and without the bias
        assert np.array_equal(_bits(e.frame_accel([eight[k]]))[:, 0], full[:, k]), k
        alone = e.frame_accel([eight[k]], bias=True)
        assert np.array_equal(_bits(alone)[:, 0], full[:, k]) and np.array_equal(_bbits(alone)[:, 0], fullb[:, k]), k
        assert np.array_equal(_bits(e.frame_accel([eight[k]], env0=3, n=1))[0, 0], full[3, k]), k
    order = (5, 0, 7, 2, 2, 1)                                                               # among other frames, in another order
    got = e.frame_accel([eight[k] for k in order], bias=True)
    for pos, k in enumerate(order):
        assert np.array_equal(_bits(got)[:, pos], full[:, k]) and np.array_equal(_bbits(got)[:, pos], fullb[:, k]), (pos, k)
    # a frame_state call between two frame_accel calls: all three as they are alone (each call keeps its own frame table)
    states = [("site", 0, dict(local=True)), ("body", nb - 1, dict(ref=("body", 1)))]
    st_alone = _sbits(e.frame_state(states))
    a1 = _bits(e.frame_accel(eight)); st = _sbits(e.frame_state(states)); a2 = _bits(e.frame_accel(eight))
    assert np.array_equal(a1, full) and np.array_equal(a2, full) and np.array_equal(st, st_alone)
    # the device form writes what the host form returns (float -> double is exact), and nothing behind its outputs
    na = NENV * 8 * 6
    ab = torch.full((na + 64,), -7.5, dtype=torch.float32, device="cuda"); bb = torch.full((na + 64,), -9.5, dtype=torch.float32, device="cuda")
    e.frame_accel_device(ab.data_ptr(), bb.data_ptr(), eight)
    e.synchronize(); torch.cuda.synchronize()
    ah, bh = ab.cpu().numpy(), bb.cpu().numpy()
    assert (ah[na:] == -7.5).all() and (bh[na:] == -9.5).all()
    a = ah[:na].reshape(NENV, 8, 6).astype(np.float64); b = bh[:na].reshape(NENV, 8, 6).astype(np.float64)
    assert np.array_equal(a[..., 0:3], with_bias["linacc"]) and np.array_equal(a[..., 3:6], with_bias["angacc"])
    assert np.array_equal(b[..., 0:3], with_bias["biasp"]) and np.array_equal(b[..., 3:6], with_bias["biasr"])
    ab.fill_(-7.5); bb.fill_(-9.5)
    e.frame_accel_device(ab.data_ptr(), None, eight, env0=2, n=2)      # no bias, a sub-range
    e.synchronize(); torch.cuda.synchronize()
    ah, bh = ab.cpu().numpy(), bb.cpu().numpy()
    assert np.array_equal(ah[:2 * 8 * 6].reshape(2, 8, 6).astype(np.float64), a[2:4]) and (ah[2 * 8 * 6:] == -7.5).all() and (bh == -9.5).all()


# ------------------------------------------------------------------ 4. physics, end to end
def _ball_model(lib, floor, z):
    """a free body with one sphere geom at its origin (centre of mass at the origin, uniform inertia), a site at the centre and one off it"""
    b = lib.mjh_builder_create()
    set_opt(lib, b, timestep=0.002)
    if floor:
        lib.mjh_builder_add_geom(b, b"floor", 0, fs.GEOM_PLANE, D(0, 0, 0.05), None, None, None, -1, -1, -1, -1)
    bd = lib.mjh_builder_add_body(b, b"ball", 0, D(0.2, -0.1, z), None, 0.0)
    lib.mjh_builder_add_joint(b, b"free", bd, fs.JNT_FREE, None, None, None, 0, 0, 0, 0, 0)
    lib.mjh_builder_add_geom(b, b"g", bd, fs.GEOM_SPHERE, D(0.1, 0, 0), None, None, None, -1, -1, -1, -1)
    lib.mjh_builder_add_site(b, b"centre", bd, D(0, 0, 0), D(*fs._unit([0.8, 0.3, -0.4, 0.2])))
    lib.mjh_builder_add_site(b, b"off", bd, D(0.03, -0.05, 0.04), D(*fs._unit([0.5, -0.6, 0.2, 0.5])))
    m = ms.Model(lib.mjh_builder_compile(b), lib); lib.mjh_builder_destroy(b)
    return m


def test_a_spinning_body_in_free_fall_reads_zero_and_the_centripetal_term(lib):
    from indep_dyn import quat2mat
    m = _ball_model(lib, floor=False, z=2.0)
    gn = float(np.linalg.norm([m.opt.gravity[k] for k in range(3)]))
    assert gn > 9
    rng = np.random.default_rng(41)
    q = np.zeros((NENV, 7)); v = np.zeros((NENV, 6))
    for i in range(NENV):
        q[i, 0:3] = [0.2, -0.1, 2.0] + rng.uniform(-0.5, 0.5, 3); q[i, 3:7] = fs._unit(rng.normal(size=4))
        v[i, 0:3] = rng.uniform(-1, 1, 3); v[i, 3:6] = rng.uniform(-4, 4, 3)
    e = ms.Engine(m, NENV)
    e.set_state(qpos=q, qvel=v, time=np.zeros(NENV), warmstart=np.zeros_like(v))
    e.forward()
    LP = dict(local=True, proper=True)
    out = e.frame_accel([("site", "centre", LP), ("site", "off", LP), ("body", "ball")])
    _, qd, vd, _ = e.get_state()
    # free fall: the classical acceleration of the centre is g, the accelerometer there reads zero; a uniform inertia has no gyroscopic
    # torque, so the angular acceleration is zero too
    s0 = gn      # |g| enters every component through PROPER
    dev0 = np.abs(out["linacc"][:, 0]).max()
    assert dev0 <= RAY_TOL * max(1.0, s0), dev0
    assert np.abs(out["angacc"]).max() <= RAY_TOL * max(1.0, s0)
    assert np.abs(out["linacc"][:, 2] - [m.opt.gravity[k] for k in range(3)]).max() <= RAY_TOL * max(1.0, s0)
    # off the centre, r in the body's axes: w x (w x r) with the body-frame angular velocity, turned into the site's axes
    r = m.array("site_pos").reshape(-1, 3)[m.name2id(3, "off")]
    S = quat2mat(m.array("site_quat").reshape(-1, 4)[m.name2id(3, "off")])
    worst = 0.0
    for i in range(NENV):
        w = vd[i, 3:6]
        want = S.T @ np.cross(w, np.cross(w, r))
        s = max(gn, np.abs(w).sum() ** 2 * np.abs(r).sum() + gn)
        worst = max(worst, np.abs(out["linacc"][i, 1] - want).max() / max(1.0, s))
    print(f"free fall: |accelerometer at the centre| {dev0:.2e}; off the centre, worst err / max(1, s) {worst:.2e} (ray rule {RAY_TOL:.0e})")
    assert worst <= RAY_TOL
    e.close()


def test_after_steps_the_call_is_ordered_behind_them_and_writes_no_state(lib):
    m = fs.rig(lib, floor=True)
    q, v, mocap = fs.states(m, NENV, seed=33, slide=0.5)
    e = ms.Engine(m, NENV)      # the default engine: cohorts, steps per launch and launch order as a user gets them
    _set(e, m, q, v, np.zeros_like(v), mocap)
    e.step(3)
    c = dict(m=m, R=far.FrameAccRef(m), frames=_every_frame(m), mocap=mocap.astype(np.float32).astype(np.float64))
    out = e.frame_accel(c["frames"], bias=True)      # queued behind the steps: no synchronise between them and the call
    before = e.get_state() + (e.get_stats(), e.get_field("qacc"))
    # a twin engine that takes the same state and steps and never issues the call: what the FIRST call left is what no call leaves
    twin = ms.Engine(m, NENV)
    _set(twin, m, q, v, np.zeros_like(v), mocap)
    twin.step(3)
    untouched = twin.get_state() + (twin.get_stats(), twin.get_field("qacc"))
    twin.close()
    for a, b in zip(untouched, before):
        assert np.array_equal(a, b)
    assert np.allclose(before[0], 3 * m.opt.timestep) and np.abs(before[5]).max() > 1      # the steps left a qacc
    _parity("rig + floor after 3 steps", c, e)
    again = e.frame_accel(c["frames"], bias=True)
    after = e.get_state() + (e.get_stats(), e.get_field("qacc"))
    for a, b in zip(before, after):      # time, qpos, qvel, warm start, statistics, qacc: bit-identical
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(out), _bits(again)) and np.array_equal(_bbits(out), _bbits(again))
    e.step(1)      # and the engine steps on
    assert np.allclose(e.get_state()[0], 4 * m.opt.timestep)
    e.close()


def test_a_sphere_resting_on_a_plane_reads_minus_gravity(lib):
    from indep_dyn import quat2mat
    m = _ball_model(lib, floor=True, z=0.1)
    g = np.array([m.opt.gravity[k] for k in range(3)]); gn = float(np.linalg.norm(g))
    q = np.tile(m.array("qpos0").astype(float), (NENV, 1))
    rng = np.random.default_rng(43)
    for i in range(NENV):
        q[i, 3:7] = fs._unit(rng.normal(size=4))
    e = ms.Engine(m, NENV)
    e.set_state(qpos=q, qvel=np.zeros((NENV, 6)), time=np.zeros(NENV), warmstart=np.zeros((NENV, 6)))
    e.step(200)
    out = e.frame_accel([("site", "centre", dict(local=True, proper=True))])
    pose = e.frame_state([("site", "centre")])
    worst = 0.0
    for i in range(NENV):
        up = quat2mat(pose["quat"][i, 0]).T @ (-g)      # the site's image of -g: world +z times |g|
        a = out["linacc"][i, 0]
        worst = max(worst, abs(np.linalg.norm(a) - gn) / gn, np.abs(a - up).max() / gn)
    print(f"sphere at rest after 200 steps: accelerometer against -g in the site's axes, worst deviation {worst:.2e} |g| (cap 1e-2)")
    assert worst <= 1e-2
    e.close()


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors_launch_nothing(lib):
    import torch
    c = _case(lib, "chain"); m, e = c["m"], c["e"]
    nb, ns = m.nbody, m.nsite
    buf = torch.full((NENV * 2 * 6 + 64,), -3.25, dtype=torch.float32, device="cuda")
    bbuf = torch.full((NENV * 2 * 6 + 64,), -4.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    F = lambda *rows: (capi.Frame * len(rows))(*[capi.Frame(*r) for r in rows])
    ok = F((0, 1, 0, -1, 0), (1, 0, 0, -1, 3))
    vp = lambda x: C.cast(x, C.c_void_p)
    call = lambda env0, n, nf, tab, acc=buf.data_ptr(), bias=bbuf.data_ptr(): lib.mjh_frame_accel_device(e.h, env0, n, nf, tab, C.c_void_p(acc), C.c_void_p(bias))
    nbig = (1 << 30) // (NENV * 6) + 1      # too many frames: the count is refused before the table is read (36 M records are not made up for it)
    assert NENV * nbig * 6 > (1 << 30) >= NENV * (nbig - 1) * 6
    bad = [call(-1, 1, 2, vp(ok)), call(0, NENV + 1, 2, vp(ok)), call(3, 3, 2, vp(ok)), call(0, 0, 2, vp(ok)),      # env range
           call(0, NENV, 0, vp(ok)), call(0, NENV, -1, vp(ok)),                                                          # nframe
           call(0, NENV, 1, vp(F((2, 0, 0, -1, 0)))), call(0, NENV, 1, vp(F((-1, 0, 0, -1, 0)))),                        # objtype
           call(0, NENV, 1, vp(F((0, nb, 0, -1, 0)))), call(0, NENV, 1, vp(F((0, -1, 0, -1, 0)))),                       # body id
           call(0, NENV, 1, vp(F((1, ns, 0, -1, 0)))), call(0, NENV, 1, vp(F((1, -1, 0, -1, 0)))),                       # site id
           call(0, NENV, 1, vp(F((0, 1, 0, 0, 0)))), call(0, NENV, 1, vp(F((0, 2, 1, 1, 2)))),                           # refid >= 0
           call(0, NENV, 1, vp(F((0, 1, 0, -2, 0)))),                                                                    # refid < -1
           call(0, NENV, 1, vp(F((0, 1, 0, -1, 4)))), call(0, NENV, 1, vp(F((0, 1, 0, -1, 7)))),                         # a flag outside LOCAL | PROPER
           call(0, NENV, 2, None), call(0, NENV, 2, vp(ok), acc=None),                                                   # null pointers
           call(0, NENV, nbig, vp(ok))]                                                                                  # n nframe 6 beyond 2^30
    assert bad == [-1] * len(bad), bad
    # mjh_frame_state keeps refusing flag 2
    sbuf = torch.full((NENV * 13 + 64,), -5.25, dtype=torch.float32, device="cuda")
    assert lib.mjh_frame_state_device(e.h, 0, NENV, 1, vp(F((0, 1, 0, -1, 2))), C.c_void_p(sbuf.data_ptr()), None) == -1
    assert lib.mjh_frame_state_device(e.h, 0, NENV, 1, vp(F((0, 1, 0, -1, 3))), C.c_void_p(sbuf.data_ptr()), None) == -1
    e.synchronize(); torch.cuda.synchronize()
    assert (buf.cpu().numpy() == -3.25).all() and (bbuf.cpu().numpy() == -4.25).all() and (sbuf.cpu().numpy() == -5.25).all()
    with pytest.raises(ms.engine.MjhError):
        e.frame_accel([("body", 1, dict(ref=("body", 2)))])
    with pytest.raises(ms.engine.MjhError):
        e.frame_accel([("site", "no such site", dict(local=True))])
    with pytest.raises(ms.engine.MjhError):
        e.frame_state([("body", 1, dict(proper=True))])
    # the smallest call works, and an error has not disturbed the frame table of the next one
    assert call(4, 1, 1, vp(F((1, ns - 1, 0, -1, 3))), bias=None) == 0
    e.synchronize(); torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = e.frame_accel([("site", ns - 1, dict(local=True, proper=True))], env0=4, n=1)
    assert np.array_equal(got[:3].astype(np.float64), want["linacc"][0, 0]) and np.array_equal(got[3:6].astype(np.float64), want["angacc"][0, 0])
    assert (got[6:] == -3.25).all() and (bbuf.cpu().numpy() == -4.25).all()


# ------------------------------------------------------------------ 6. Engine.imu
def test_imu_is_one_frame_state_and_one_frame_accel_call(lib):
    c = _case(lib, "rig"); m, e = c["m"], c["e"]
    sites = ["s_root", "s_tip", "s_ball", "s_free", "s_mocap"]
    imu = e.imu(sites)
    st = e.frame_state([("site", s, dict(local=True)) for s in sites])
    ac = e.frame_accel([("site", s, dict(local=True, proper=True)) for s in sites])
    assert sorted(imu) == ["accel", "gyro", "quat"] and imu["accel"].shape == (NENV, 5, 3) and imu["quat"].shape == (NENV, 5, 4)
    assert np.array_equal(imu["quat"].view(np.int64), st["quat"].view(np.int64))
    assert np.array_equal(imu["gyro"].view(np.int64), st["angvel"].view(np.int64))
    assert np.array_equal(imu["accel"].view(np.int64), ac["linacc"].view(np.int64))
    assert np.abs(imu["accel"]).max() > 1      # not vacuous
    sub = e.imu([m.name2id(3, "s_tip")], env0=2, n=2)      # ids and a sub-range
    assert np.array_equal(sub["accel"][:, 0], imu["accel"][2:4, 1]) and np.array_equal(sub["gyro"][:, 0], imu["gyro"][2:4, 1])
