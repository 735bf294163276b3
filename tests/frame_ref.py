"""frame_ref.py — TEST INFRASTRUCTURE: pose, twist and Jacobian of bodies and sites in numpy fp64, the yardstick of mjh_frame_state.

Built on indep_dyn.Tree.fk and the joint columns it returns (dof, "lin" | "rot", world axis, world anchor): a frame's Jacobian at its world
origin p has, for every column of its body and of the body's ancestors,

    lin:  jacp = axis,               jacr = 0
    rot:  jacp = axis x (p - anchor), jacr = axis

and zeros elsewhere; linvel = jacp qvel, angvel = jacr qvel.  A site adds its offset: p = xpos[b] + R_b site_pos, q = xquat[b] * site_quat.
Mocap bodies take the pose given per env (they have no dofs).  The ref / LOCAL rules are applied as include/mjhip.h states them:

    LOCAL:  linvel, angvel <- R^T linvel, R^T angvel          (the frame's own axes; the pose stays the world pose)
    ref:    pos = Rr^T (p - pr),  quat = qr^-1 q,  linvel = Rr^T (v - vr - wr x (p - pr)),  angvel = Rr^T (w - wr)

A frame is (objtype, id, reftype, refid, flags) with objtype / reftype 0 body, 1 site, refid -1 for none and flags & 1 LOCAL.
tests/test_frame_ref.py checks all of this against finite differences of the forward kinematics alone."""
import numpy as np

from indep_dyn import Tree, quat2mat, mulquat

BODY, SITE, LOCAL = 0, 1, 1


def conj(q):
    return np.array([q[0], -q[1], -q[2], -q[3]])


class FrameRef:
    def __init__(self, m):
        self.tree = Tree(m)
        self.nv, self.nb = m.nv, m.nbody
        self.site_body = m.array("site_bodyid").astype(int)
        self.site_pos = m.array("site_pos").reshape(-1, 3).astype(float)
        self.site_quat = m.array("site_quat").reshape(-1, 4).astype(float)
        mid = m.array("body_mocapid").astype(int) if m.nmocap else np.zeros(0, int)
        self.mocapid = mid if len(mid) else -np.ones(m.nbody, int)
        self.nmocap = m.nmocap
        par = self.tree.par
        self.chain = []                      # bodies from b up to (not including) the world
        for b in range(self.nb):
            c, a = [], b
            while a > 0:
                c.append(a); a = par[a]
            self.chain.append(c)

    def depth(self, objtype, i):
        """bodies in the frame's chain (at least 1)"""
        return max(1, len(self.chain[self.body_of(objtype, i)]))

    def body_of(self, objtype, i):
        return int(self.site_body[i]) if objtype == SITE else int(i)

    def fk(self, q, mocap=None):
        """body poses and joint columns; mocap [nmocap, 7] (pos, quat) replaces the pose of mocap bodies"""
        xpos, xquat, cols = self.tree.fk(np.asarray(q, float))
        if self.nmocap and mocap is not None:
            mocap = np.asarray(mocap, float).reshape(-1, 7)
            for b in range(self.nb):
                if self.mocapid[b] >= 0:
                    xpos[b] = mocap[self.mocapid[b], :3]; xquat[b] = mocap[self.mocapid[b], 3:]
        return xpos, xquat, cols

    def pose(self, fk, objtype, i):
        xpos, xquat, _ = fk
        if objtype == SITE:
            b = self.site_body[i]
            return xpos[b] + quat2mat(xquat[b]) @ self.site_pos[i], mulquat(xquat[b], self.site_quat[i])
        return xpos[i].copy(), xquat[i].copy()

    def jacobian_at(self, fk, body, p):
        """world Jacobian [6, nv] (rows 0-2 jacp, 3-5 jacr) of the point p carried by `body`"""
        J = np.zeros((6, self.nv))
        for a in self.chain[body]:
            for (d, kind, axis, anchor) in fk[2][a]:
                if kind == "lin":
                    J[0:3, d] = axis
                else:
                    J[0:3, d] = np.cross(axis, p - anchor); J[3:6, d] = axis
        return J

    def world(self, fk, v, objtype, i):
        """world pose, twist and Jacobian of one frame"""
        p, q = self.pose(fk, objtype, i)
        J = self.jacobian_at(fk, self.body_of(objtype, i), p)
        return p, q, J[0:3] @ v, J[3:6] @ v, J

    def evaluate(self, q, v, frames, mocap=None):
        """-> dict of pos [nf, 3], quat [nf, 4], linvel, angvel [nf, 3], jac [nf, 6, nv] (always world), and for the error scales
        sv [nf, 6] = sum_d |col_d| |qvel_d| of the reported twist's terms (the frame's, plus the ref's where one is given)"""
        v = np.asarray(v, float)
        fk = self.fk(q, mocap)
        nf = len(frames)
        out = dict(pos=np.zeros((nf, 3)), quat=np.zeros((nf, 4)), linvel=np.zeros((nf, 3)), angvel=np.zeros((nf, 3)),
                   jac=np.zeros((nf, 6, self.nv)), sv=np.zeros((nf, 6)))
        for k, (objtype, i, reftype, refid, flags) in enumerate(frames):
            p, qq, lin, ang, J = self.world(fk, v, objtype, i)
            sv = np.abs(J) @ np.abs(v)
            if refid >= 0:
                assert not flags & LOCAL
                pr, qr, linr, angr, Jr = self.world(fk, v, reftype, refid)
                R = quat2mat(qr)
                dp = p - pr
                lin = R.T @ (lin - linr - np.cross(angr, dp)); ang = R.T @ (ang - angr)
                svr = np.abs(Jr) @ np.abs(v)
                sv = sv + svr
                sv[0:3] += np.abs(np.cross(np.eye(3), dp)) @ svr[3:6]      # the terms of wr x dp
                sv[0:3] = np.abs(R.T) @ sv[0:3]; sv[3:6] = np.abs(R.T) @ sv[3:6]
                p = R.T @ dp; qq = mulquat(conj(qr), qq)
            elif flags & LOCAL:
                R = quat2mat(qq)
                lin = R.T @ lin; ang = R.T @ ang
                sv[0:3] = np.abs(R.T) @ sv[0:3]; sv[3:6] = np.abs(R.T) @ sv[3:6]
            out["pos"][k] = p; out["quat"][k] = qq; out["linvel"][k] = lin; out["angvel"][k] = ang; out["jac"][k] = J; out["sv"][k] = sv
        return out


def frame_tuple(model, item):
    """("body" | "site", name_or_id[, dict(ref=(type, name_or_id), local=bool)]) -> (objtype, id, reftype, refid, flags)"""
    def one(kind, ref):
        t = dict(body=BODY, site=SITE)[kind]
        return t, (model.name2id(0 if t == BODY else 3, ref) if isinstance(ref, str) else int(ref))
    opt = item[2] if len(item) > 2 else {}
    t, i = one(*item[:2])
    rt, ri = one(*opt["ref"]) if opt.get("ref") is not None else (0, -1)
    assert i >= 0 and (ri >= 0 or opt.get("ref") is None), item
    return t, i, rt, ri, LOCAL if opt.get("local") else 0
