"""The yardstick of the frame-acceleration tests (tests/frame_acc_ref.py) against central finite differences of FrameRef's own twist, on
the CPU:

    acc  ~  [twist(integrate(q, v, +h), v + h qacc) - twist(integrate(q, v, -h), v - h qacc)] / 2h          bias: the same with qacc = 0

twist = (linvel, angvel) of frame_ref.FrameRef.evaluate, which tests/test_frame_ref.py pins to the forward kinematics.  The path
q(+-h) = integrate(q, v, +-h) differs from the true motion by (h^2 / 2) qacc, the same on both sides, so it drops out of the central
difference to O(h^2) like the difference's own truncation.

Choice of h and of the tolerance.  The twist varies on the time scale 1 / W of the tree's angular rates, W <= sum |qvel| over a chain's
rotations: the central difference's truncation is (h^2 / 6) |f'''| ~ (h W)^2 |f'| / 6, its rounding 2^-52 |f| / h ~ 2^-52 |f'| / (h W).
With the states below (|qvel| <= 2, |qacc| <= 5: W up to ~30 on the rig and ~100 along the 70-dof chain) the two meet near
h = (6 2^-52)^(1/3) / W ~ 1e-7 .. 1e-6; h = 1e-6 leaves (h W)^2 / 6 <= 2e-9 and 2^-52 / (h W) <= 1e-10 relative to the size of the
terms, which the reference's scale s (the sum of the absolute products) measures.  TOL = 1e-7 max(1, s) stands a factor ~50 above that
estimate and seven orders below the size of a wrong or missing term.
Observed worst |err| / max(1, s) with these seeds: rig 1.7e-10 (acc) and 4.4e-10 (bias), chain70 1.3e-10 (acc) and 5.5e-10 (bias)."""
import numpy as np
import pytest

import frame_ref as fr
import frame_acc_ref as far
import frame_scenes as fs
from indep_dyn import quat2mat

H = 1e-6
TOL = 1e-7


def _all_frames(m, flags=0):
    return [(fr.BODY, b, flags) for b in range(m.nbody)] + [(fr.SITE, s, flags) for s in range(m.nsite)]


@pytest.fixture(scope="module", params=["rig", "chain70"])
def case(request, lib):
    m = dict(rig=lambda: fs.rig(lib), chain70=lambda: fs.chain(lib, (70,)))[request.param]()
    q, v, mocap = fs.states(m, 2, slide=0.5 if request.param == "rig" else 0.05)
    qacc = np.random.default_rng(5).uniform(-5, 5, v.shape)
    return request.param, m, far.FrameAccRef(m), q, v, qacc, mocap


def _twist_fd(R, q, v, qacc, frames, mocap):
    five = [(t, j, 0, -1, 0) for (t, j, _) in frames]
    tr = R.tree
    tw = []
    for sgn in (1, -1):
        o = R.evaluate(tr.integrate(q, v, sgn * H), v + sgn * H * qacc, five, mocap)
        tw.append(np.concatenate([o["linvel"], o["angvel"]], axis=1))
    return (tw[0] - tw[1]) / (2 * H)


def test_acc_and_bias_are_the_central_difference_of_the_twist(case):
    name, m, R, q, v, qacc, mocap = case
    frames = _all_frames(m)
    worst = dict(acc=0.0, bias=0.0)
    for i in range(len(q)):
        ref = R.evaluate_acc(q[i], v[i], qacc[i], frames, mocap[i])
        acc = np.concatenate([ref["linacc"], ref["angacc"]], axis=1); bias = np.concatenate([ref["biasp"], ref["biasr"]], axis=1)
        ea = np.abs(acc - _twist_fd(R, q[i], v[i], qacc[i], frames, mocap[i])) / np.maximum(1.0, ref["s"])
        eb = np.abs(bias - _twist_fd(R, q[i], v[i], 0 * qacc[i], frames, mocap[i])) / np.maximum(1.0, ref["sb"])
        worst["acc"] = max(worst["acc"], ea.max()); worst["bias"] = max(worst["bias"], eb.max())
        # acc - bias = J qacc with FrameRef's own Jacobian
        five = [(t, j, 0, -1, 0) for (t, j, _) in frames]
        J = R.evaluate(q[i], v[i], five, mocap[i])["jac"]
        assert np.abs(acc - bias - J @ qacc[i]).max() <= 1e-12 * max(1.0, np.abs(acc).max())
        # the scale bounds the value, and a component without terms is zero
        assert (np.abs(acc) <= ref["s"] * (1 + 1e-12)).all() and (np.abs(bias) <= ref["sb"] * (1 + 1e-12)).all()
    print(f"[{name}] worst |reference - central difference| / max(1, s): acc {worst['acc']:.2e}, bias {worst['bias']:.2e} (TOL {TOL:.0e}, h {H:.0e})")
    assert worst["acc"] <= TOL and worst["bias"] <= TOL, worst


def test_local_and_proper_rules(case):
    name, m, R, q, v, qacc, mocap = case
    g = R.gravity
    assert np.abs(g).max() > 1      # the models have gravity: PROPER is not vacuous
    plain = _all_frames(m)
    flags = (0, fr.LOCAL, far.PROPER, fr.LOCAL | far.PROPER)
    for i in range(len(q)):
        every = R.evaluate_acc(q[i], v[i], qacc[i], [f for fl in flags for f in _all_frames(m, fl)], mocap[i])
        o = {fl: {key: val[n * len(plain):(n + 1) * len(plain)] for key, val in every.items()} for n, fl in enumerate(flags)}
        fk = R.fk(q[i], mocap[i])
        for k, (t, j, _) in enumerate(plain):
            Rk = quat2mat(R.pose(fk, t, j)[1])
            lin, ang = o[0]["linacc"][k], o[0]["angacc"][k]
            assert np.allclose(o[far.PROPER]["linacc"][k], lin - g, rtol=0, atol=1e-12) and np.array_equal(o[far.PROPER]["angacc"][k], ang)
            assert np.allclose(o[fr.LOCAL]["linacc"][k], Rk.T @ lin, rtol=0, atol=1e-12) and np.allclose(o[fr.LOCAL]["angacc"][k], Rk.T @ ang, rtol=0, atol=1e-12)
            assert np.allclose(o[fr.LOCAL | far.PROPER]["linacc"][k], Rk.T @ (lin - g), rtol=0, atol=1e-12)
            for fl in o:      # the bias ignores the flags
                assert np.array_equal(o[fl]["biasp"][k], o[0]["biasp"][k]) and np.array_equal(o[fl]["biasr"][k], o[0]["biasr"][k])
        # LOCAL | PROPER against the central difference of the WORLD twist, turned into the frame's own axes: the accelerometer reads
        # R^T (d2p/dt2 - g), not the derivative of the velocimeter's R^T v
        fd = _twist_fd(R, q[i], v[i], qacc[i], plain, mocap[i])
        lp = o[fr.LOCAL | far.PROPER]
        for k, (t, j, _) in enumerate(plain):
            Rk = quat2mat(R.pose(fk, t, j)[1])
            want = np.concatenate([Rk.T @ (fd[k, 0:3] - g), Rk.T @ fd[k, 3:6]])
            got = np.concatenate([lp["linacc"][k], lp["angacc"][k]])
            assert (np.abs(got - want) <= TOL * np.maximum(1.0, lp["s"][k])).all(), (name, i, t, j)


def test_world_and_mocap_read_zero_or_minus_g(lib):
    m = fs.rig(lib)
    R = far.FrameAccRef(m)
    q, v, mocap = fs.states(m, 1, slide=0.5)
    qacc = np.random.default_rng(6).uniform(-5, 5, v.shape)
    mc, smc = m.name2id(0, "mc"), m.name2id(3, "s_mocap")
    fk = R.fk(q[0], mocap[0])
    for (t, j) in ((fr.BODY, 0), (fr.BODY, mc), (fr.SITE, smc)):
        o = R.evaluate_acc(q[0], v[0], qacc[0], [(t, j, 0), (t, j, far.PROPER), (t, j, fr.LOCAL | far.PROPER)], mocap[0])
        assert not o["linacc"][0].any() and not o["angacc"].any() and not o["biasp"].any() and not o["biasr"].any() and not o["s"][0].any()
        assert np.array_equal(o["linacc"][1], -R.gravity) and np.array_equal(o["s"][1][0:3], np.abs(R.gravity))
        assert np.allclose(o["linacc"][2], quat2mat(R.pose(fk, t, j)[1]).T @ -R.gravity, rtol=0, atol=1e-14)
    # a model with gravity disabled subtracts nothing
    R0 = far.FrameAccRef(m, gravity=[0, 0, 0])
    o = R0.evaluate_acc(q[0], v[0], qacc[0], [(fr.BODY, mc, far.PROPER)], mocap[0])
    assert not o["linacc"].any()
