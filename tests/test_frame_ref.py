"""The yardstick of the frame-state tests (tests/frame_ref.py) against finite differences of the forward kinematics alone, on the CPU:
the reference Jacobian of every body and site frame equals the central-difference Jacobian of the frame's pose along
Tree.integrate(q, +-eps e_d) (indep_dyn.jacobians_fd's scheme, extended to a site point); twist = J qvel; the ref and LOCAL rules equal
the finite difference of the relative (resp. own-axes) pose along integrate(q, +-eps qvel)."""
import numpy as np
import pytest

import frame_ref as fr
import frame_scenes as fs
from indep_dyn import quat2mat

EPS = 1e-6
TOL = 2e-7      # central differences at eps = 1e-6 of poses of size <= ~4: truncation eps^2 |f'''| / 6 and rounding 1e-16 |f| / eps, both below 1e-8


def _vee(S):
    return np.array([S[2, 1] - S[1, 2], S[0, 2] - S[2, 0], S[1, 0] - S[0, 1]])


def _all_frames(m):
    return [(fr.BODY, b, 0, -1, 0) for b in range(m.nbody)] + [(fr.SITE, s, 0, -1, 0) for s in range(m.nsite)]


@pytest.fixture(scope="module", params=["rig", "chain70", "chain6+64"])
def case(request, lib):
    m = dict(rig=lambda: fs.rig(lib), chain70=lambda: fs.chain(lib, (70,)), **{"chain6+64": lambda: fs.chain(lib, (6, 64))})[request.param]()
    q, v, mocap = fs.states(m, 2, slide=0.5 if request.param == "rig" else 0.05)
    return m, fr.FrameRef(m), q, v, mocap


def test_models_have_the_shapes_the_tests_are_about(lib):
    m = fs.rig(lib)
    jt = m.array("jnt_type"); root = m.name2id(0, "root")
    assert m.array("body_jntnum")[root] == 3 and m.nmocap == 1 and m.nsite == 5
    assert sorted(jt.tolist()).count(fs.JNT_BALL) == 1 and sorted(jt.tolist()).count(fs.JNT_FREE) == 1
    assert m.array("body_mocapid")[m.name2id(0, "mc")] == 0
    c = fs.chain(lib, (70,))
    assert c.nv == 70 and c.ntree == 1 and c.nbody == 71
    c = fs.chain(lib, (6, 64))
    assert c.nv == 70 and list(c.array("tree_dofnum")) == [6, 64] and list(c.array("tree_dofadr")) == [0, 6]


def test_jacobian_is_the_central_difference_of_the_pose(case):
    m, R, q, v, mocap = case
    frames = _all_frames(m)
    tr = R.tree
    for i in range(len(q)):
        ref = R.evaluate(q[i], v[i], frames, mocap[i])
        Jfd = np.zeros((len(frames), 6, m.nv))
        for d in range(m.nv):
            e = np.zeros(m.nv); e[d] = 1
            fp, fm = R.fk(tr.integrate(q[i], e, EPS), mocap[i]), R.fk(tr.integrate(q[i], e, -EPS), mocap[i])
            for k, (t, j, _, _, _) in enumerate(frames):
                (pp, qp), (pm, qm) = R.pose(fp, t, j), R.pose(fm, t, j)
                Jfd[k, 0:3, d] = (pp - pm) / (2 * EPS)
                Jfd[k, 3:6, d] = _vee(quat2mat(qp) @ quat2mat(qm).T) / (4 * EPS)
        assert np.abs(ref["jac"] - Jfd).max() <= TOL, np.abs(ref["jac"] - Jfd).max()
        # twist = J qvel
        assert np.abs(ref["linvel"] - ref["jac"][:, 0:3] @ v[i]).max() <= 1e-13 and np.abs(ref["angvel"] - ref["jac"][:, 3:6] @ v[i]).max() <= 1e-13
        # columns outside the chain are zero; a mocap body has none
        da, dn = m.array("body_dofadr"), m.array("body_dofnum")
        for k, (t, j, _, _, _) in enumerate(frames):
            mine = set(d for a in R.chain[R.body_of(t, j)] for d in range(da[a], da[a] + dn[a]))
            assert not ref["jac"][k][:, [d for d in range(m.nv) if d not in mine]].any()
            assert len(mine) > 0 or not (ref["linvel"][k].any() or ref["angvel"][k].any())


def _pairs(m):
    """(frame, ref) pairs: every site and a few bodies against a ref on the same tree, on another tree and a site ref"""
    nb, ns = m.nbody, m.nsite
    out = []
    for s in range(ns):
        out += [(fr.SITE, s, fr.BODY, 1, 0), (fr.SITE, s, fr.BODY, nb - 1, 0), (fr.SITE, s, fr.SITE, (s + 1) % ns, 0), (fr.SITE, s, fr.SITE, s, 0)]
    for b in (1, nb // 2, nb - 1):
        out += [(fr.BODY, b, fr.SITE, 0, 0), (fr.BODY, b, fr.BODY, max(1, b - 1), 0), (fr.BODY, b, fr.BODY, 0, 0)]
    return out


def test_ref_and_local_rules_are_the_finite_difference_of_the_relative_pose(case):
    m, R, q, v, mocap = case
    tr = R.tree
    rel = _pairs(m)
    loc = [(t, j, 0, -1, fr.LOCAL) for (t, j, _, _, _) in _all_frames(m)]
    for i in range(len(q)):
        out = R.evaluate(q[i], v[i], rel + loc, mocap[i])
        op, om = (R.evaluate(tr.integrate(q[i], v[i], s * EPS), v[i], rel + loc, mocap[i]) for s in (1, -1))
        n = len(rel)
        lin_fd = (op["pos"] - om["pos"]) / (2 * EPS)
        assert np.abs(out["linvel"][:n] - lin_fd[:n]).max() <= TOL * max(1, np.abs(lin_fd).max())
        for k in range(len(rel) + len(loc)):
            S = quat2mat(op["quat"][k]) @ quat2mat(om["quat"][k]).T      # = exp([2 eps w]x), w in the axes the quaternion maps INTO
            w = _vee(S) / (4 * EPS)
            if k < n:
                assert np.abs(out["angvel"][k] - w).max() <= TOL * max(1, np.abs(w).max()), (k, out["angvel"][k], w)
            else:      # LOCAL: the world pose is reported; its derivative, turned into the frame's own axes
                Rk = quat2mat(out["quat"][k])
                assert np.abs(out["linvel"][k] - Rk.T @ lin_fd[k]).max() <= TOL * max(1, np.abs(lin_fd[k]).max())
                assert np.abs(out["angvel"][k] - Rk.T @ w).max() <= TOL * max(1, np.abs(w).max())
        # a frame relative to itself: at the origin, at rest
        for k, (t, j, rt, rj, _) in enumerate(rel):
            if (t, j) == (rt, rj):
                assert not out["pos"][k].any() and not out["linvel"][k].any() and not out["angvel"][k].any()
                # (|q|^2 of a product of up to ~140 unit quaternions, every product within a few 2^-52 of unit length)
                assert np.abs(out["quat"][k] - [1, 0, 0, 0]).max() <= 1e-12
