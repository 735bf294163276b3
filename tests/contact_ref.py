"""fp64 numpy reference of the contact report, built from oracle FIELDS alone (efc_force, efc_type, efc_id, efc_J, the contacts, poses,
xfrc_applied) and the model's tables — not from the oracle's own cfrc_ext code:

  contact_forces  per contact, the force in the contact frame on geom2's body: normal, tangent 1, tangent 2, torque about the normal
                  (mj_contactForce for condim <= 4), decoded from the contact's pyramid rows;
  cfrc_ext        per body, torque(3) force(3) in world axes about the subtree COM of the body's tree root: xfrc_applied, the contact
                  forces and the connect / weld rows;
  body_sums       net contact force on selected bodies in world axes, optionally only from contacts against a given body.

Test infrastructure only."""
import numpy as np

CNSTR_EQUALITY, CNSTR_FRICTIONLESS, CNSTR_PYRAMIDAL = 0, 5, 6
EQ_CONNECT, EQ_WELD, EQ_JOINT = 0, 1, 2


def contact_rows(d, ic):
    """indices of the constraint rows of contact ic"""
    ty, ids = d.ifield("efc_type"), d.ifield("efc_id")
    return np.nonzero(((ty == CNSTR_FRICTIONLESS) | (ty == CNSTR_PYRAMIDAL)) & (ids == ic))[0]


def contact_mu(m, con):
    """friction of a contact's pyramid bases (tangent 1, tangent 2, torsional): the geoms' maximum"""
    fr = np.asarray(m.array("geom_friction"), dtype=np.float64).reshape(-1, 3)
    g1, g2 = con["geom"]
    mx = np.maximum(fr[g1], fr[g2])
    return np.array([mx[0], mx[0], mx[1]])


def contact_forces(m, d, cons=None):
    """[ncon, 4]; a contact without rows has zero force"""
    cons = d.contacts() if cons is None else cons
    f = d.f("efc_force")
    out = np.zeros((len(cons), 4))
    for ic, c in enumerate(cons):
        rows = contact_rows(d, ic)
        if len(rows) == 0:
            continue
        if c["dim"] == 1:
            out[ic, 0] = f[rows[0]]
            continue
        assert len(rows) == 2 * (c["dim"] - 1), (ic, c["dim"], rows)
        mu = contact_mu(m, c)
        for k in range(1, c["dim"]):      # base k: rows 2(k-1) (+) and 2(k-1)+1 (-)
            fp, fm = f[rows[2 * (k - 1)]], f[rows[2 * (k - 1) + 1]]
            out[ic, 0] += fp + fm
            out[ic, k] += mu[k - 1] * (fp - fm)
    return out


def world_force(con, cf):
    """contact-frame force (normal, tangent 1, tangent 2) -> world axes: frame^T cf (the frame's rows are the axes)"""
    R = np.asarray(con["frame"], dtype=np.float64).reshape(3, 3)
    return R.T @ np.asarray(cf[:3], dtype=np.float64)


def qfrc_from_decoded(m, d, cons=None):
    """J^T f with every contact's rows replaced by its DECODED force on the normal / tangent Jacobians recovered from efc_J
    (Jn = (J+ + J-) / 2, Jt = (J+ - J-) / (2 mu)); equals qfrc_constraint iff the decoding is right"""
    cons = d.contacts() if cons is None else cons
    nefc = d.i("nefc"); f = d.f("efc_force")
    nv = d.f("qvel").shape[0]
    J = d.f("efc_J").reshape(nefc, nv)
    cf = contact_forces(m, d, cons)
    used = np.zeros(nefc, dtype=bool)
    q = np.zeros(nv)
    for ic, c in enumerate(cons):
        rows = contact_rows(d, ic)
        used[rows] = True
        if len(rows) == 0:
            continue
        if c["dim"] == 1:
            q += cf[ic, 0] * J[rows[0]]
            continue
        mu = contact_mu(m, c)
        Jn = 0.5 * (J[rows[0]] + J[rows[1]])
        q += cf[ic, 0] * Jn
        for k in range(1, c["dim"]):
            Jt = (J[rows[2 * (k - 1)]] - J[rows[2 * (k - 1) + 1]]) / (2.0 * mu[k - 1])
            q += cf[ic, k] * Jt
    for i in np.nonzero(~used)[0]:
        q += f[i] * J[i]
    return q


def _mulquat(a, b):
    return np.array([a[0]*b[0] - a[1]*b[1] - a[2]*b[2] - a[3]*b[3], a[0]*b[1] + a[1]*b[0] + a[2]*b[3] - a[3]*b[2],
                     a[0]*b[2] - a[1]*b[3] + a[2]*b[0] + a[3]*b[1], a[0]*b[3] + a[1]*b[2] - a[2]*b[1] + a[3]*b[0]])


def cfrc_ext(m, d, cons=None):
    """[nbody, 6]"""
    cons = d.contacts() if cons is None else cons
    nb = m.nbody
    root = np.asarray(m.array("body_rootid")); gb = np.asarray(m.array("geom_bodyid"))
    com = d.f("subtree_com").reshape(nb, 3); xipos = d.f("xipos").reshape(nb, 3)
    xpos = d.f("xpos").reshape(nb, 3); xmat = d.f("xmat").reshape(nb, 3, 3); xquat = d.f("xquat").reshape(nb, 4)
    out = np.zeros((nb, 6))

    def add(b, point, force, torque, sign):
        if b <= 0:
            return
        off = np.asarray(point) - com[root[b]]
        out[b, :3] += sign * (np.asarray(torque) + np.cross(off, force))
        out[b, 3:] += sign * np.asarray(force)

    xf = d.f("xfrc_applied").reshape(nb, 6)
    for b in range(1, nb):
        add(b, xipos[b], xf[b, :3], xf[b, 3:], 1.0)
    cf = contact_forces(m, d, cons)
    for ic, c in enumerate(cons):
        F = world_force(c, cf[ic]); T = np.asarray(c["frame"][:3]) * cf[ic, 3]
        add(gb[c["geom"][1]], c["pos"], F, T, 1.0)
        add(gb[c["geom"][0]], c["pos"], F, T, -1.0)
    ty, ids, f = d.ifield("efc_type"), d.ifield("efc_id"), d.f("efc_force")
    eqt = np.asarray(m.array("eq_type")) if m.neq else np.zeros(0, dtype=int)
    i = 0
    z3 = np.zeros(3)
    while i < d.i("nefc"):
        if ty[i] != CNSTR_EQUALITY or eqt[ids[i]] == EQ_JOINT:
            i += 1
            continue
        e = ids[i]; weld = eqt[e] == EQ_WELD
        b1, b2 = int(m.array("eq_obj1id")[e]), int(m.array("eq_obj2id")[e])
        dat = np.asarray(m.array("eq_data"), dtype=np.float64)[11 * e:11 * e + 11]
        a1, a2 = (dat[3:6], dat[0:3]) if weld else (dat[0:3], dat[3:6])
        p1 = xpos[b1] + xmat[b1] @ a1; p2 = xpos[b2] + xmat[b2] @ a2
        add(b1, p1, f[i:i + 3], z3, 1.0); add(b2, p2, f[i:i + 3], z3, -1.0)
        if weld:      # rows 3..5: cpos' = A (w2 - w1): torque A^T f on body2, -A^T f on body1
            q1i = xquat[b1] * np.array([1.0, -1.0, -1.0, -1.0]); q2r = _mulquat(xquat[b2], dat[6:10])
            T = np.zeros(3)
            for a in range(3):
                w = np.zeros(4); w[1 + a] = 1.0
                v = _mulquat(_mulquat(q1i, w), q2r)
                T[a] = 0.5 * dat[10] * (v[1:4] @ f[i + 3:i + 6])
            add(b2, p2, z3, T, 1.0); add(b1, p1, z3, T, -1.0)
        i += 6 if weld else 3
    return out


def body_sums(m, cons, cf, bodies, against=None):
    """([nsel, 3] net contact force ON each body in world axes, [nsel] contacts in each sum); cons / cf: contacts (dicts with frame and
    geom) and their contact-frame forces [ncon, >= 3], from the oracle or from a device report"""
    gb = np.asarray(m.array("geom_bodyid"))
    bodies = np.atleast_1d(bodies)
    against = -np.ones(len(bodies), dtype=int) if against is None else np.broadcast_to(np.atleast_1d(against), bodies.shape)
    F = np.zeros((len(bodies), 3)); cnt = np.zeros(len(bodies), dtype=int)
    for c, f in zip(cons, cf):
        b1, b2 = gb[c["geom"][0]], gb[c["geom"][1]]
        w = world_force(c, f)
        for s, (b, a) in enumerate(zip(bodies, against)):
            if b2 == b and (a < 0 or b1 == a):
                F[s] += w; cnt[s] += 1
            elif b1 == b and (a < 0 or b2 == a):
                F[s] -= w; cnt[s] += 1
    return F, cnt
