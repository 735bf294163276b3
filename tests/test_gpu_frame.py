"""Frame states on the device (mjh_frame_state / mjh_frame_state_device, csrc/frame.hip) against the numpy fp64 reference of
tests/frame_ref.py, evaluated at the device's OWN fp32 state (read back by get_state; mocap poses rounded to fp32): only the frame
arithmetic is under test, not the stepper.  Models and states: tests/frame_scenes.py, 5 envs with different states.

Parity bound:  err <= C 2^-23 depth s,  depth = bodies in the frame's chain (plus the ref's where one is given),
    pose:           s = max(1, |p|inf) (of the frame's and the ref's world position); quaternion components with the same s
    twist:          s = sum_d |col_d| |qvel_d| per component, from the reference (a ref adds its own terms and those of wr x (p - pr))
    Jacobian entry: s = max(1, |col|inf) of its column
C is four times the worst ratio measured on the MI355X over the cases here, rounded up to a power of two (the margin is for other seeds).
Measured worst err / (2^-23 depth s):
    rig (17 dofs: odom joints, hinges, ball, free, mocap)      pose 1.32, twist  3.90, Jacobian 1.05
    rig with a floor, after three steps                        pose 0.99, twist  2.72, Jacobian 1.79
    chains of 6 and 64 dofs (nv = 70)                          pose 0.85, twist 11.01, Jacobian 0.84
so C = 64 (4 x 11.01 = 44, rounded up).  The chain model is compact, and its chains' first joints sit at the body origin, for the reason
tests/frame_scenes.py gives: the twist scale has no term for the rounding of the levers, and read 98 and 667 on less compact chains.
Independently of C every pose and twist component also satisfies the ray rule |err| <= 5e-5 max(1, s) (tests/ray_check.py).

Identities on the device's own output are held to summation rounding, nchain 2^-23 sum|terms|, derived in place."""
import ctypes as C

import numpy as np
import pytest

import mujoco_sim_amd as ms
from mujoco_sim_amd import capi
import frame_ref as fr
import frame_scenes as fs
import ray_check

pytestmark = pytest.mark.gpu
NENV = 5
EPS = 2.0 ** -23
C_BOUND = 64.0
RAY_TOL = ray_check.TOL


# ------------------------------------------------------------------ models, states, engines and frame lists: made once, never changed
_CACHE = {}


def _rig_frames(m):
    """every body (the world and the mocap body included) and site, world and LOCAL; refs on the same tree, on another tree, site refs,
    a mocap ref, a frame against itself"""
    B = lambda n: ("body", n)
    S = lambda n: ("site", n)
    plain = [("body", b) for b in range(m.nbody)] + [("site", s) for s in range(m.nsite)]
    local = [(t, i, dict(local=True)) for t, i in plain]
    refs = [S("s_tip") + (dict(ref=B("root")),), S("s_ball") + (dict(ref=B("l2")),), B("l4") + (dict(ref=B("l1")),),      # same tree
            S("s_free") + (dict(ref=B("root")),), S("s_tip") + (dict(ref=B("fb")),), B("bl2") + (dict(ref=B("fb")),),     # another tree
            B("l4") + (dict(ref=S("s_root")),), S("s_tip") + (dict(ref=S("s_free")),), S("s_ball") + (dict(ref=S("s_tip")),),   # site refs
            S("s_tip") + (dict(ref=S("s_mocap")),), B("mc") + (dict(ref=B("root")),), S("s_root") + (dict(ref=B(0)),),
            S("s_tip") + (dict(ref=S("s_tip")),), B("fb") + (dict(ref=B("fb")),)]
    return plain + local + refs


def _chain_frames(m):
    nb = m.nbody
    bodies = [0, 1, 5, 6, 7, 8, 37, 38, 63, 64, 65, nb - 2, nb - 1]
    plain = [("body", b) for b in bodies] + [("site", s) for s in range(m.nsite)]
    local = [(t, i, dict(local=True)) for t, i in plain[3:]]
    refs = [("site", m.nsite - 1, dict(ref=("body", 7))), ("body", nb - 1, dict(ref=("body", nb - 2))), ("site", m.nsite - 1, dict(ref=("site", m.nsite - 2))),
            ("site", m.nsite - 1, dict(ref=("body", 6))), ("body", 3, dict(ref=("site", m.nsite - 1))), ("site", 0, dict(ref=("site", m.nsite - 1)))]
    return plain + local + refs


def _case(lib, name):
    if name in _CACHE:
        return _CACHE[name]
    if name == "rig":
        m = fs.rig(lib); q, v, mocap = fs.states(m, NENV, slide=0.5); frames = _rig_frames(m)
    else:
        m = fs.chain(lib, (6, 64)); q, v, mocap = fs.states(m, NENV); frames = _chain_frames(m)
        assert m.nv == 70 and list(m.array("tree_dofadr")) == [0, 6]      # the long chain's dofs lie on both passes of the stride loop
    e = ms.Engine(m, NENV)
    _set(e, m, q, v, mocap)
    _CACHE[name] = dict(m=m, e=e, R=fr.FrameRef(m), frames=frames, mocap=mocap.astype(np.float32).astype(np.float64))
    return _CACHE[name]


def _set(e, m, q, v, mocap):
    e.set_state(qpos=q, qvel=v, time=np.zeros(len(q)), warmstart=np.zeros_like(v))
    for k in range(m.nmocap):
        e.set_mocap_pose(k, mocap[:, k, :3], mocap[:, k, 3:])


def _parity(name, c, e=None):
    """the device's frame states of every env against the reference at the device's own state; returns the worst ratios"""
    m, R, frames = c["m"], c["R"], c["frames"]
    e = e or c["e"]
    _, qd, vd, _ = e.get_state()
    out = e.frame_state(frames, jacobian=True)
    tup = [fr.frame_tuple(m, f) for f in frames]
    worst = dict(pose=0.0, twist=0.0, jac=0.0, ray=0.0)
    for i in range(NENV):
        fk = R.fk(qd[i], c["mocap"][i])
        ref = R.evaluate(qd[i], vd[i], tup, c["mocap"][i])
        for k, (t, j, rt, rj, fl) in enumerate(tup):
            depth = R.depth(t, j) + (R.depth(rt, rj) if rj >= 0 else 0)
            pw = [R.pose(fk, t, j)[0]] + ([R.pose(fk, rt, rj)[0]] if rj >= 0 else [])
            sp = max(1.0, max(np.abs(p).max() for p in pw))
            ep = max(np.abs(out["pos"][i, k] - ref["pos"][k]).max(), np.abs(out["quat"][i, k] - ref["quat"][k]).max())
            dev_tw = np.concatenate([out["linvel"][i, k], out["angvel"][i, k]]); ref_tw = np.concatenate([ref["linvel"][k], ref["angvel"][k]])
            et = np.abs(dev_tw - ref_tw); sv = ref["sv"][k]
            assert (et[sv == 0] == 0).all(), (name, i, frames[k], dev_tw, ref_tw)      # no terms: exactly zero
            J = np.concatenate([out["jacp"][i, k], out["jacr"][i, k]]); Jr = ref["jac"][k]
            ej = np.abs(J - Jr).max(axis=0) / np.maximum(1.0, np.abs(Jr).max(axis=0))
            worst["pose"] = max(worst["pose"], ep / (EPS * depth * sp))
            worst["twist"] = max(worst["twist"], (et[sv > 0] / (EPS * depth * sv[sv > 0])).max() if (sv > 0).any() else 0.0)
            worst["jac"] = max(worst["jac"], ej.max() / (EPS * R.depth(t, j)) if m.nv else 0.0)
            worst["ray"] = max(worst["ray"], ep / sp, (et / np.maximum(1.0, sv)).max())
    print(f"[{name}] worst err / (2^-23 depth s): pose {worst['pose']:.2f}, twist {worst['twist']:.2f}, Jacobian {worst['jac']:.2f}; "
          f"worst err / max(1, s): {worst['ray']:.2e} (ray rule {RAY_TOL:.0e}); C = {C_BOUND}")
    assert worst["ray"] <= RAY_TOL, (name, worst)
    assert max(worst["pose"], worst["twist"], worst["jac"]) <= C_BOUND, (name, worst)
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
    out = e.frame_state(plain, jacobian=True)
    _, qd, vd, _ = e.get_state()
    xpos, xquat = e.get_body_state()
    da, dn = m.array("body_dofadr"), m.array("body_dofnum")
    sb = m.array("site_bodyid")
    worst = dict(twist=0.0, site=0.0)
    for i in range(NENV):
        fk = R.fk(qd[i], c["mocap"][i])
        for k, (t, j) in enumerate(plain):
            b = R.body_of(fr.SITE if t == "site" else fr.BODY, j)
            mine = sorted(d for a in R.chain[b] for d in range(da[a], da[a] + dn[a]))
            J = np.concatenate([out["jacp"][i, k], out["jacr"][i, k]])
            # columns outside the chain are exactly zero
            assert not J[:, [d for d in range(m.nv) if d not in mine]].any(), (name, i, t, j)
            # twist = J qvel, formed in fp64 from the device's Jacobian and qvel: len(mine) products and additions in fp32
            tw = np.concatenate([out["linvel"][i, k], out["angvel"][i, k]])
            bound = max(len(mine), 1) * EPS * (np.abs(J) @ np.abs(vd[i]))
            err = np.abs(tw - J @ vd[i])
            assert (err <= bound).all(), (name, i, t, j, err, bound)
            worst["twist"] = max(worst["twist"], (err[bound > 0] / bound[bound > 0]).max() if (bound > 0).any() else 0.0)
            if t == "body":      # the pose the position stage exported, as get_body_state reads it
                assert np.array_equal(out["pos"][i, k], xpos[i, j]) and np.array_equal(out["quat"][i, k], xquat[i, j]), (name, i, j)
            else:
                # a site and its body: the same angular velocity (bitwise), v_site = v_body + w x (p_site - p_body).  Both sides sum, per
                # rotational column, products of the axis (|axis| <= 1) with a lever — p_site - anchor, p_body - anchor, p_site - p_body —
                # times qvel: one rounding for the lever, two for a cross product's component, one for the product with qvel, and up to
                # len(mine) for the sums; the levers' sizes from the reference's anchors
                kb = sb[j]
                assert np.array_equal(out["angvel"][i, k], out["angvel"][i, kb]) and np.array_equal(out["jacr"][i, k], out["jacr"][i, kb])
                dp = out["pos"][i, k] - out["pos"][i, kb]
                terms = 0.0
                for a in R.chain[b]:
                    for (d, kind, axis, anchor) in fk[2][a]:
                        if kind == "rot":
                            terms += abs(vd[i, d]) * (np.abs(out["pos"][i, k] - anchor).sum() + np.abs(out["pos"][i, kb] - anchor).sum() + np.abs(dp).sum())
                bound = (len(mine) + 4) * EPS * terms
                err = np.abs(out["linvel"][i, k] - (out["linvel"][i, kb] + np.cross(out["angvel"][i, kb], dp))).max()
                assert err <= bound, (name, i, j, err, bound)
                worst["site"] = max(worst["site"], err / bound if bound > 0 else 0.0)
    print(f"[{name}] identities, worst error / bound: twist = J qvel {worst['twist']:.2f}, site against its body {worst['site']:.2f}")
    if name == "rig":
        mc, smc = m.name2id(0, "mc"), m.name2id(3, "s_mocap")
        for k in (mc, m.nbody + smc):      # the mocap body and its site: the pose set per env, zero twist, a zero Jacobian
            assert not out["linvel"][:, k].any() and not out["angvel"][:, k].any() and not out["jacp"][:, k].any() and not out["jacr"][:, k].any()
        assert np.array_equal(out["pos"][:, mc], c["mocap"][:, 0, :3]) and np.array_equal(out["quat"][:, mc], c["mocap"][:, 0, 3:])
    # a frame with ref = itself: the same walk twice, so zero position and twist; the quaternion is |q|^2 (unit to a few roundings)
    selfref = [(t, j, dict(ref=(t, j))) for t, j in plain]
    o2 = e.frame_state(selfref)
    assert not o2["pos"].any() and not o2["linvel"].any() and not o2["angvel"].any()
    assert np.abs(o2["quat"] - [1, 0, 0, 0]).max() <= 8 * EPS, np.abs(o2["quat"] - [1, 0, 0, 0]).max()


# ------------------------------------------------------------------ 3. bitwise independence
def _bits(d):
    return np.concatenate([d[k] for k in ("pos", "quat", "linvel", "angvel")], axis=-1).view(np.int64)


@pytest.mark.parametrize("name", ["rig", "chain"])
def test_a_frame_does_not_depend_on_the_call_around_it(name, lib):
    import torch
    c = _case(lib, name); m, e = c["m"], c["e"]
    ns, nb = m.nsite, m.nbody
    eight = [("site", ns - 1), ("body", nb - 1, dict(local=True)), ("site", ns - 1, dict(ref=("body", 1))), ("body", 1), ("site", 0, dict(local=True)),
             ("body", nb // 2, dict(ref=("site", ns - 1))), ("site", ns - 1, dict(ref=("site", 0))), ("body", nb - 1)]
    full = _bits(e.frame_state(eight, jacobian=True))
    assert np.array_equal(_bits(e.frame_state(eight)), full)                              # without the Jacobian output
    assert np.array_equal(_bits(e.frame_state(eight, env0=3, n=1, jacobian=True))[0], full[3])      # another range
    assert np.array_equal(_bits(e.frame_state(eight, env0=1, n=3))[2], full[3])
    for k in (0, 2, 5):                                                                     # alone in a call, with and without the Jacobian
        for jac in (False, True):
            assert np.array_equal(_bits(e.frame_state([eight[k]], jacobian=jac))[:, 0], full[:, k]), (k, jac)
        assert np.array_equal(_bits(e.frame_state([eight[k]], env0=3, n=1))[0, 0], full[3, k]), k
    shuffled = [eight[k] for k in (5, 0, 7, 2, 2, 1)]                                       # among other frames, in another order
    got = _bits(e.frame_state(shuffled, jacobian=True))
    for pos, k in enumerate((5, 0, 7, 2, 2, 1)):
        assert np.array_equal(got[:, pos], full[:, k]), (pos, k)
    # the device form writes what the host form returns (float -> double is exact), and nothing behind its outputs
    host = e.frame_state(eight, jacobian=True)
    nst, nj = NENV * 8 * 13, NENV * 8 * 6 * m.nv
    st = torch.full((nst + 64,), -7.5, dtype=torch.float32, device="cuda"); jb = torch.full((nj + 64,), -9.5, dtype=torch.float32, device="cuda")
    e.frame_state_device(st.data_ptr(), jb.data_ptr(), eight)
    e.synchronize(); torch.cuda.synchronize()
    sh, jh = st.cpu().numpy(), jb.cpu().numpy()
    assert (sh[nst:] == -7.5).all() and (jh[nj:] == -9.5).all()
    s = sh[:nst].reshape(NENV, 8, 13).astype(np.float64); J = jh[:nj].reshape(NENV, 8, 6, m.nv).astype(np.float64)
    assert np.array_equal(s[..., 0:3], host["pos"]) and np.array_equal(s[..., 3:7], host["quat"]) and np.array_equal(s[..., 7:10], host["linvel"])
    assert np.array_equal(s[..., 10:13], host["angvel"]) and np.array_equal(J[:, :, 0:3], host["jacp"]) and np.array_equal(J[:, :, 3:6], host["jacr"])
    st.fill_(-7.5)
    e.frame_state_device(st.data_ptr(), None, eight, env0=2, n=2)      # no Jacobian, a sub-range
    e.synchronize(); torch.cuda.synchronize()
    sh = st.cpu().numpy()
    assert np.array_equal(sh[:2 * 8 * 13].reshape(2, 8, 13).astype(np.float64), s[2:4]) and (sh[2 * 8 * 13:] == -7.5).all()


# ------------------------------------------------------------------ 4. after stepping
def test_after_steps_the_call_is_ordered_behind_them_and_writes_no_state(lib):
    m = fs.rig(lib, floor=True)
    q, v, mocap = fs.states(m, NENV, seed=33, slide=0.5)
    e = ms.Engine(m, NENV)      # the default engine: cohorts, steps per launch and launch order as a user gets them
    _set(e, m, q, v, mocap)
    e.step(3)
    c = dict(m=m, R=fr.FrameRef(m), frames=_rig_frames(m), mocap=mocap.astype(np.float32).astype(np.float64))
    out = e.frame_state(c["frames"])      # queued behind the steps: no synchronise between them and the call
    before = e.get_state() + (e.get_stats(),)
    assert np.allclose(before[0], 3 * m.opt.timestep)
    w = _parity("rig + floor after 3 steps", c, e)
    again = e.frame_state(c["frames"])
    after = e.get_state() + (e.get_stats(),)
    for a, b in zip(before, after):      # time, qpos, qvel, warm start, statistics: bit-identical
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(out), _bits(again))
    e.step(1)      # and the engine steps on
    assert np.allclose(e.get_state()[0], 4 * m.opt.timestep)
    e.close()


# ------------------------------------------------------------------ 5. argument errors
def test_argument_errors_launch_nothing(lib):
    import torch
    c = _case(lib, "chain"); m, e = c["m"], c["e"]
    nb, ns, nv = m.nbody, m.nsite, m.nv
    buf = torch.full((NENV * 2 * 13 + 64,), -3.25, dtype=torch.float32, device="cuda")
    jbuf = torch.full((NENV * 2 * 6 * nv + 64,), -3.25, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    F = lambda *rows: (capi.Frame * len(rows))(*[capi.Frame(*r) for r in rows])
    ok = F((0, 1, 0, -1, 0), (1, 0, 0, -1, 0))
    vp = lambda x: C.cast(x, C.c_void_p)
    call = lambda env0, n, nf, tab, st=buf.data_ptr(), jac=None: lib.mjh_frame_state_device(e.h, env0, n, nf, tab, C.c_void_p(st), C.c_void_p(jac))
    big = np.zeros(((1 << 30) // (NENV * 6 * nv) + 1, 5), dtype=np.int32); big[:, 3] = -1      # valid frames (body 0, no ref), too many of them
    assert C.sizeof(capi.Frame) == big.strides[0]
    bad = [call(-1, 1, 2, vp(ok)), call(0, NENV + 1, 2, vp(ok)), call(3, 3, 2, vp(ok)), call(0, 0, 2, vp(ok)),      # env range
           call(0, NENV, 0, vp(ok)), call(0, NENV, -1, vp(ok)),                                                          # nframe
           call(0, NENV, 1, vp(F((2, 0, 0, -1, 0)))), call(0, NENV, 1, vp(F((-1, 0, 0, -1, 0)))),                        # objtype
           call(0, NENV, 1, vp(F((0, nb, 0, -1, 0)))), call(0, NENV, 1, vp(F((0, -1, 0, -1, 0)))),                       # body id
           call(0, NENV, 1, vp(F((1, ns, 0, -1, 0)))), call(0, NENV, 1, vp(F((1, -1, 0, -1, 0)))),                       # site id
           call(0, NENV, 1, vp(F((0, 1, 0, nb, 0)))), call(0, NENV, 1, vp(F((0, 1, 1, ns, 0)))),                         # ref id
           call(0, NENV, 1, vp(F((0, 1, 2, 0, 0)))), call(0, NENV, 1, vp(F((0, 1, 0, -2, 0)))),                          # reftype, refid < -1
           call(0, NENV, 1, vp(F((0, 1, 0, 2, 1)))), call(0, NENV, 1, vp(F((0, 1, 0, -1, 2)))),                          # LOCAL with a ref, unknown flag
           call(0, NENV, 2, None), call(0, NENV, 2, vp(ok), st=None),                                                    # null pointers
           call(0, NENV, len(big), C.c_void_p(big.ctypes.data), jac=jbuf.data_ptr())]                                                       # n nframe 6 nv beyond 2^30
    assert bad == [-1] * len(bad), bad
    e.synchronize(); torch.cuda.synchronize()
    assert (buf.cpu().numpy() == -3.25).all() and (jbuf.cpu().numpy() == -3.25).all()
    with pytest.raises(ms.engine.MjhError, match=r"\(-1\)"):
        e.frame_state([("body", 1, dict(ref=("body", 2), local=True))])
    with pytest.raises(ms.engine.MjhError):
        e.frame_state([("site", "no such site")])
    # the smallest call works, and an error has not disturbed the frame table of the next one
    assert call(4, 1, 1, vp(F((1, ns - 1, 0, -1, 0)))) == 0
    e.synchronize(); torch.cuda.synchronize()
    got = buf.cpu().numpy()
    want = e.frame_state([("site", ns - 1)], env0=4, n=1)
    assert np.array_equal(got[:3].astype(np.float64), want["pos"][0, 0]) and np.array_equal(got[10:13].astype(np.float64), want["angvel"][0, 0])
    assert (got[13:] == -3.25).all()


def test_engines_are_closed(lib):
    for c in _CACHE.values():
        c["e"].close()
    _CACHE.clear()
