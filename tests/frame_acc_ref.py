"""frame_acc_ref.py — TEST INFRASTRUCTURE: classical acceleration and bias (Jdot qvel) of bodies and sites in numpy fp64, the yardstick of
mjh_frame_accel.  Built on frame_ref.FrameRef (poses, chains and the joint columns of indep_dyn.Tree.fk).

The Jacobian column of dof d at the frame's world origin p is c_d = (a_d, 0) for a translation and (a_d x (p - r_d), a_d) for a rotation
(axis a_d, anchor r_d).  The reference differentiates every column along every dof's own motion, pair by pair, with no staging:

    H[:, d, e] = d c_d / d q_e                      (e, d in the chain of the frame's body; "q_e" in the velocity sense)
    da   = a_e x a_d          if e is a rotation of a joint in FRONT of d's joint (the frame a_d is fixed in turns with it), else 0
    dp   = c_e(p)             (p is carried by every dof of the chain)
    dr_d = c_e(r_d)  if e < d (the anchor is carried by the dofs in front of d; zero for the rotations of d's own ball or free joint, whose
                               anchor it is; a free joint's translations move its anchor), else 0
    translation d:  H = (da, 0)            rotation d:  H = (da x (p - r_d) + a_d x (dp - dr_d),  da)

The three columns of a ball or free joint turn with the body's full angular velocity, their own joint's included; that adds a_e x a_d for
the pairs (d, e) of ONE joint — antisymmetric in (d, e), so its sum against qvel_d qvel_e is exactly zero, and it is left out.

    bias = sum_{d,e} H[:, d, e] qvel_d qvel_e   (= Jdot qvel)            acc = J qacc + bias
    PROPER: linacc <- linacc - gravity          LOCAL: both vectors <- R^T vector (after PROPER); the bias stays as it is

Scale s per component, for the error bound of the GPU test: the sum of the absolute values of every elementary product that enters the
component — |J| |qacc|, and for every pair the cross products taken term by term (abscross(x, y)_i = |x_j y_k| + |x_k y_j|) times
|qvel_d qvel_e| — plus |gravity| per component with PROPER; LOCAL maps it through |R^T|.  A component with s = 0 has no term at all.
What s has no term for (as the twist scale of tests/test_gpu_frame.py, see tests/frame_scenes.py): an fp32 evaluation forms the levers
p - r_d from coordinates that are themselves rounded at 2^-24 of THEIR size, so a lever much shorter than |p| carries a relative error far
above 2^-23.  `lever` = sum over the chain's rotations of abscross(a_d, |p| + |r_d|) |qacc_d| measures that input (a diagnostic the GPU
test prints beside its ratios; no bound uses it; measured on the rig and chain models it does not lower the ratios).  `axis` = sum over the
chain of |qacc_d| (angular part, and translations' linear part) and abscross(1, p - r_d) |qacc_d| (rotations' linear part): the size of
an absolute 2^-24 error per component of a unit axis, a second diagnostic of the same kind.
tests/test_frame_acc_ref.py checks all of this against finite differences of FrameRef's own twist."""
import numpy as np

from frame_ref import FrameRef, BODY, SITE, LOCAL
from indep_dyn import quat2mat

PROPER = 2


def abscross(x, y):
    """|x_j y_k| + |x_k y_j| per component i (rows of 3-vectors broadcast): the cross product's two products, in absolute value"""
    x, y = np.asarray(x, float), np.asarray(y, float)
    return np.abs(np.roll(x, -1, -1) * np.roll(y, -2, -1)) + np.abs(np.roll(x, -2, -1) * np.roll(y, -1, -1))


class FrameAccRef(FrameRef):
    def __init__(self, m, gravity=None):
        super().__init__(m)
        g = np.array([m.opt.gravity[k] for k in range(3)], float) if gravity is None else np.asarray(gravity, float)
        self.gravity = np.zeros(3) if (m.opt.disableflags & (1 << 6)) else g      # MJH_DSBL_GRAVITY
        self.dof_jnt = m.array("dof_jntid").astype(int)

    def _columns(self, fk, body):
        """the chain's columns in ascending dof order: (d, is_rot, axis, anchor, joint)"""
        cols = [(d, kind == "rot", np.asarray(axis, float), None if anchor is None else np.asarray(anchor, float), self.dof_jnt[d])
                for a in self.chain[body] for (d, kind, axis, anchor) in fk[2][a]]
        return sorted(cols, key=lambda c: c[0])

    def hessian_at(self, fk, body, p):
        """H [6, nv, nv] and its scale SH (sums of absolute elementary products) of the point p carried by `body`"""
        nv = self.nv
        H = np.zeros((6, nv, nv)); SH = np.zeros((6, nv, nv))
        cols = self._columns(fk, body)
        if not cols:
            return H, SH
        # the columns e as arrays (one row per chain dof); a translation's anchor is unused
        E = np.array([c[0] for c in cols]); RE = np.array([c[1] for c in cols]); AE = np.array([c[2] for c in cols])
        NE = np.array([c[3] if c[1] else np.zeros(3) for c in cols]); JE = np.array([c[4] for c in cols])
        ab = abscross
        rot = RE[:, None]
        dp = np.where(rot, np.cross(AE, p - NE), AE); sdp = np.where(rot, ab(AE, p - NE), np.abs(AE))
        for (d, rd, ad, anc_d, jd) in cols:
            front = (RE & (E < d) & (JE != jd))[:, None]
            da = np.where(front, np.cross(AE, ad), 0.0); sda = np.where(front, ab(AE, ad[None]), 0.0)
            if not rd:
                H[0:3, d, E] = da.T; SH[0:3, d, E] = sda.T
                continue
            before = (E < d)[:, None]
            dr = np.where(before, np.where(rot, np.cross(AE, anc_d - NE), AE), 0.0)
            sdr = np.where(before, np.where(rot, ab(AE, anc_d - NE), np.abs(AE)), 0.0)
            H[0:3, d, E] = (np.cross(da, p - anc_d) + np.cross(ad, dp - dr)).T
            SH[0:3, d, E] = (ab(sda, (p - anc_d)[None]) + ab(ad[None], sdp) + ab(ad[None], sdr)).T
            H[3:6, d, E] = da.T; SH[3:6, d, E] = sda.T
        return H, SH

    def evaluate_acc(self, q, v, qacc, frames, mocap=None):
        """frames: (objtype, id, flags) or frame_ref's five-tuples with refid -1 -> dict of linacc, angacc, biasp, biasr [nf, 3] and the
        scales s [nf, 6] (of acc, flags applied) and sb [nf, 6] (of the bias); lever [nf, 6]: see the module's last paragraph"""
        v = np.asarray(v, float); qacc = np.asarray(qacc, float)
        fk = self.fk(q, mocap)
        nf = len(frames)
        out = dict(linacc=np.zeros((nf, 3)), angacc=np.zeros((nf, 3)), biasp=np.zeros((nf, 3)), biasr=np.zeros((nf, 3)),
                   s=np.zeros((nf, 6)), sb=np.zeros((nf, 6)), lever=np.zeros((nf, 6)), axis=np.zeros((nf, 6)))
        vv = np.outer(v, v)
        done = {}      # a frame listed again with other flags: its sums are formed once
        for k, fr in enumerate(frames):
            objtype, i, flags = (fr[0], fr[1], fr[-1])
            assert len(fr) == 3 or fr[3] < 0, "accelerations have no ref-relative form"
            p, qq = self.pose(fk, objtype, i)
            body = self.body_of(objtype, i)
            if (objtype, i) not in done:
                J = self.jacobian_at(fk, body, p)
                H, SH = self.hessian_at(fk, body, p)
                bias = np.einsum("rde,de->r", H, vv); sb = np.einsum("rde,de->r", SH, np.abs(vv))
                lever = np.zeros(6); axis = np.zeros(6)
                for (d, rd, ad, anc_d, _) in self._columns(fk, body):
                    if rd:
                        lever[0:3] += abscross(ad, np.abs(p) + np.abs(anc_d)) * abs(qacc[d])
                        axis[0:3] += abscross(np.ones(3), p - anc_d) * abs(qacc[d]); axis[3:6] += abs(qacc[d])
                    else:
                        axis[0:3] += abs(qacc[d])
                done[(objtype, i)] = (J @ qacc + bias, np.abs(J) @ np.abs(qacc) + sb, bias, sb, lever, axis)
            acc, s, bias, sb, lever, axis = (x.copy() for x in done[(objtype, i)])
            if flags & PROPER:
                acc[0:3] -= self.gravity; s[0:3] += np.abs(self.gravity)
            if flags & LOCAL:
                R = quat2mat(qq)
                acc = np.concatenate([R.T @ acc[0:3], R.T @ acc[3:6]])
                s = np.concatenate([np.abs(R.T) @ s[0:3], np.abs(R.T) @ s[3:6]])
                lever = np.concatenate([np.abs(R.T) @ lever[0:3], lever[3:6]])
                axis = np.concatenate([np.abs(R.T) @ axis[0:3], np.abs(R.T) @ axis[3:6]])
            out["linacc"][k] = acc[0:3]; out["angacc"][k] = acc[3:6]; out["biasp"][k] = bias[0:3]; out["biasr"][k] = bias[3:6]
            out["s"][k] = s; out["sb"][k] = sb; out["lever"][k] = lever; out["axis"][k] = axis
        return out


def accel_tuple(model, item):
    """("body" | "site", name_or_id[, dict(local=bool, proper=bool)]) -> (objtype, id, flags)"""
    opt = item[2] if len(item) > 2 else {}
    t = dict(body=BODY, site=SITE)[item[0]]
    i = model.name2id(0 if t == BODY else 3, item[1]) if isinstance(item[1], str) else int(item[1])
    assert i >= 0 and not set(opt) - {"local", "proper"}, item
    return t, i, (LOCAL if opt.get("local") else 0) | (PROPER if opt.get("proper") else 0)
