"""Every solver form of the device against the certified optimum of its constraint program (tests/qp_ref.py).

The constrained accelerations of a step are the unique solution of a strictly convex, bound-constrained QP (R > 0), so with the sweep
cap lifted (5000 sweeps, tolerance 0) every form — whatever its order, schedule or storage — must reach the same point.  Pattern of
test_gpu_round5.py's _qp_check, through the public API only: a second engine with the default options brings the scene to a state, the
engine under test takes that state, steps once and returns its qacc (the next warm start); the oracle, with ONE sweep, assembles the
program of the same step (J, AR, b, the row kinds), qp_ref solves it and certifies the solution by its KKT residual.  No PGS of the
oracle takes part.  An instance counts where the device's contact and row counts are the oracle's and the certificate holds.

Asserted for every form: at least 80 % of the env-states handed to the oracle count, at least 8 of them, and the relative qacc error
(max |delta| / max(1, max |ref|)) is <= 1e-3 at the median instance and <= 1e-2 at the worst — the project's bound for an fp32 fixed
point against the fp64 optimum (the window kernel's, test_gpu_round5.py).  tests/test_qp_ref.py shows what that bound catches.

Out: the noslip post-pass.  It drops R from the rows it re-solves, so what it returns is not this program's optimum."""
import os

import numpy as np
import pytest

import mujoco_sim_amd as ms
import orc
import qp_ref
from helpers import load_model_tables, oracle_s24
from test_robot_fixtures import robot_command

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MEDIAN, WORST = 1e-3, 1e-2
CLASSES = ((1, 128), (129, 192), (193, 256))          # rows: the dense sweeps keep two / three / four rows per lane


def _lifted(m):
    m.c.opt.iterations = 5000; m.c.opt.tolerance = 0.0
    return m


class Sample:
    """one state of every env (as get_state returns it), the command of the step that follows, and per env the certified reference
    of that step: (ncon, nefc, qacc*) or None"""

    def __init__(self, e, cmd=None, with_inverse=False):
        self.t, self.q, self.v, self.w = e.get_state()
        self.cmd, self.inv = cmd, with_inverse
        self.ref = [None] * e.nenv
        self.keep = None          # per env: the dofs that are compared (all, unless set)
        self.handed = 0

    def rows(self, d, i):
        """the oracle (opt.iterations = 1) takes env i's state and the command and steps once, whole stage order -> its row count"""
        d.f("qpos")[:] = self.q[i]; d.f("qvel")[:] = self.v[i]; d.f("qacc_warmstart")[:] = self.w[i]; d.f("qacc")[:] = self.w[i]; d.f("time")[0] = self.t[i]
        if self.cmd is not None:
            d.f("ddq")[:] = self.cmd[i]
        d.step(1, int(self.inv))
        return d.i("nefc")

    def certify(self, d, mo, i):
        """... and its program, solved and certified (an instance without the certificate is not an instance)"""
        self.handed += 1
        if d.i("nefc") == 0:
            return
        AR, b, J, lo, hi = qp_ref.assemble(d, mo)
        f, res = qp_ref.solve(AR, b, lo, hi)
        if qp_ref.certified(AR, b, res):
            qacc = qp_ref.qacc_of(d, J, f)
            self.ref[i] = (d.i("ncon"), d.i("nefc"), qacc if self.keep is None else qacc[self.keep[i]])

    def reference(self, d, mo, envs=None):
        for i in (range(len(self.ref)) if envs is None else envs):
            self.rows(d, i); self.certify(d, mo, i)
        return self


def _device(e, samples):
    """the engine under test takes each sample's state, steps once -> (rows, error, sweeps) of the instances that count, instances handed over"""
    out, handed = [], 0
    for s in samples:
        e.set_state(qpos=s.q, qvel=s.v, time=s.t, warmstart=s.w)
        if s.cmd is not None:
            e.set_cmd(ddq=s.cmd)
        e.step(1, s.inv)
        _, _, _, qacc = e.get_state(); st = e.get_stats()
        handed += s.handed
        for i, r in enumerate(s.ref):
            if r is None or r[0] != st[i, 0] or r[1] != st[i, 1] or (st[i, 3] & 7):
                continue                                        # (another contact set: fp32 / fp64 narrow phase at a margin)
            out.append((r[1], qp_ref.rel_err(qacc[i] if s.keep is None else qacc[i][s.keep[i]], r[2]), st[i, 2]))
    return np.array(out).reshape(-1, 3), handed


def _line(label, rec):
    if not len(rec):
        return f"QP-FORM {label}: no instance"
    return (f"QP-FORM {label}: {len(rec)} instances, {int(rec[:, 0].min())}..{int(rec[:, 0].max())} rows, sweeps mean {rec[:, 2].mean():.0f}: "
            f"qacc rel error median {np.median(rec[:, 1]):.2e} 99% {np.quantile(rec[:, 1], 0.99):.2e} max {rec[:, 1].max():.2e}")


def _assert_form(label, rec, handed, min_rows=0):
    print(_line(label, rec) + f" ({len(rec)} of {handed} handed to the oracle)")
    assert len(rec) >= 8 and len(rec) >= 0.8 * handed, label
    assert rec[:, 0].max() >= min_rows, label
    assert np.median(rec[:, 1]) <= MEDIAN and rec[:, 1].max() <= WORST, label


def _yawed(q0, nbody, rng, amp, first=0):
    """free bodies' poses turned about the world's z axis through their own centres by up to +- amp rad: the envs are not copies"""
    q = q0.copy()
    for k in range(first, nbody):
        a = rng.uniform(-amp, amp); c, s = np.cos(a / 2), np.sin(a / 2)
        w, x, y, z = q[7 * k + 3:7 * k + 7]
        q[7 * k + 3:7 * k + 7] = [c * w - s * z, c * x - s * y, c * y + s * x, c * z + s * w]
    return q


# ---------------------------------------------------------------- the robots: dense row-space solver, block solver, LDS-resident sweeps
def _robot(name):
    return load_model_tables(os.path.join(G, f"robot_{name}.npz"))


def _c4_slots(m):
    names = [m.lib.mjh_id2name(m.ptr, 0, b).decode() for b in range(m.c.nbody)]
    return [b for b, n in enumerate(names) if n.startswith("object_")], (m.c.nbody - 32 if m.c.nbody > 32 else 0)


def _c4_engine(m, z, nenv):
    """C4's fixture, env i with i % 9 pool objects in play (the slot masks of test_dense_sweeps_of_every_row_class…)"""
    e = ms.Engine(m, nenv)
    e.set_controlled_dofs(z["controlled"].astype(np.int32))
    slots, sbase = _c4_slots(m)
    mask = []
    for b in slots:
        e.set_slot_active(b, False)
    for i in range(nenv):
        mk = 0
        for j, b in enumerate(slots):
            if j < i % (len(slots) + 1):
                e.set_slot_active(b, True, env0=i, n=1)
            else:
                mk |= 1 << (b - sbase)
        mask.append(mk)
    return e, mask


_C4 = {}


def _c4_samples():
    """72 envs, the objects released beside the robot, each in its own sector of the ring around it: objects released INTO each other
    (15 cm deep with random angles) are generic-convex pairs whose portal refinement is ill-conditioned — fp32 and fp64 normals 4 degrees
    apart, another program with the same row count, on which all three forms agreed with each other to three digits and missed the
    oracle's optimum by 0.17.  After every 6-step stretch envs are handed to the oracle (chosen by the row count of
    the device's last step, classed by the oracle's own) until each row class of the dense sweeps has 12, so that 8 remain where fp32 and
    fp64 contact sets differ.  The last class fills once most of 7 or 8 objects have landed (from step ~80 on).  The dofs of parked pool
    objects are left out of the comparison: a parked body is held (qacc 0 on both sides), qacc_smooth + M^-1 J'f is its free fall.
    Computed once, shared by the tests of the dense form, the block solver and the capacity fall-back."""
    if "samples" in _C4:
        return _C4["samples"], _C4["mo"]
    nenv = 72
    ms_, z = _robot("c4_pr2_world_objects_mesh"); mo, _ = _robot("c4_pr2_world_objects_mesh")
    es, mask = _c4_engine(ms_, z, nenv)
    slots, _ = _c4_slots(ms_)
    rng = np.random.default_rng(606)
    for i in range(nenv):
        for j in range(i % (len(slots) + 1)):
            a, r = 2 * np.pi * (j + rng.uniform(0.4, 0.6)) / len(slots) - np.pi, rng.uniform(0.9, 1.4)          # (each object in its own sector)
            quat = rng.normal(size=4); quat /= np.linalg.norm(quat)
            es.set_body_pose(i, slots[j], np.array([r * np.sin(a), r * np.cos(a), rng.uniform(0.15, 0.5)]), quat, np.array([0.1, -0.1, -0.3, *(0.5 * rng.normal(size=3))]))
    mo.c.opt.iterations = 1
    ds = []
    for i in range(nenv):
        d = orc.OrcData(mo.ptr); d.ifield("controlled")[:] = z["controlled"]
        orc.lib().orc_set_slot_mask(d.d, mask[i]); ds.append(d)
    scale = rng.uniform(0.5, 1.5, size=(nenv, 1))
    dof_body = [int(b) for b in ms_.array("dof_bodyid")]; sbase = _c4_slots(ms_)[1]
    keep = [np.array([not (b >= sbase and (mask[i] >> (b - sbase)) & 1) for b in dof_body]) for i in range(nenv)]
    cls = lambda n: next((c for c in CLASSES if c[0] <= n <= c[1]), None)
    have = {c: 0 for c in CLASSES}
    samples = []; step = 0
    for rep in range(28):
        for k in range(6):
            step += 1
            es.set_cmd(ddq=robot_command(ms_, step) * scale); es.step(1, True)
        step += 1
        s = Sample(es, robot_command(ms_, step) * scale, True); s.keep = keep
        last = es.get_stats()[:, 1]
        want = dict(have); took = {c: 0 for c in CLASSES}
        for i in range(nenv):
            c = cls(last[i])
            if c is None or want[c] >= 12 or took[c] >= 4:          # (at most four of a class from one point in time)
                continue
            want[c] += 1; took[c] += 1
            c = cls(s.rows(ds[i], i))
            if c is not None:
                s.certify(ds[i], mo, i); have[c] += 1
        if s.handed:
            samples.append(s)
        if min(have.values()) >= 12:
            break
        es.set_cmd(ddq=s.cmd); es.step(1, True)
    es.close()
    _C4.update(samples=samples, mo=mo, z=z)
    return samples, mo


def _c4_form(form, monkeypatch):
    """(rows, error, sweeps) of C4's samples through one form: 'dense', 'block' (MJH_DENSE=0), 'cap64' (MJH_DENSE_CAP=64)"""
    if form in _C4:
        return _C4[form]
    samples, _ = _c4_samples()
    if form == "block":
        monkeypatch.setenv("MJH_DENSE", "0")
    if form == "cap64":
        monkeypatch.setenv("MJH_DENSE_CAP", "64")
    m, z = _robot("c4_pr2_world_objects_mesh")
    e, _ = _c4_engine(_lifted(m), z, 72)
    monkeypatch.delenv("MJH_DENSE", raising=False); monkeypatch.delenv("MJH_DENSE_CAP", raising=False)
    assert e.dense_solver() == (0 if form == "block" else 1)
    _C4[form] = _device(e, samples)
    e.close()
    return _C4[form]


def _by_class(rec):
    return {c: rec[(rec[:, 0] >= c[0]) & (rec[:, 0] <= c[1])] for c in CLASSES}


def test_dense_sweeps_two_three_and_four_rows_per_lane(monkeypatch):
    """csrc/dense_pgs.h, AR = Y D^-1 Y' from the matrix cores, column-scaled in visiting order, swept with two (<= 128 rows), three
    (129 - 192) and four (193 - 256) rows per lane: equality rows of the PR2's joint couplings (f free), joint limits and pyramidal
    contacts of the robot and of 0 .. 8 landing objects.  Each row class has its own line and its own floor of 8 instances."""
    rec, handed = _c4_form("dense", monkeypatch)
    by = _by_class(rec)
    for c, r in by.items():
        print(_line(f"dense, {c[0]}-{c[1]} rows (K = {(c[1] + 63) // 64})", r))
    for c, r in by.items():
        assert len(r) >= 8, (c, len(r))
        assert np.median(r[:, 1]) <= MEDIAN and r[:, 1].max() <= WORST, c
    _assert_form("dense K = 2, 3, 4 (C4)", rec, handed, 193)
    # measured (MI355X, 5000 sweeps; median / 99 % / max): two rows per lane 12 of 12 instances, 107 .. 123 rows, 3.0e-5 / 5.8e-5 / 5.9e-5; three 14 of 14,
    # 129 .. 192 rows, 1.5e-5 / 5.4e-5 / 5.4e-5; four 12 of 12, 196 .. 216 rows, 1.3e-5 / 1.3e-4 / 1.4e-4; all 38: 1.9e-5 / 1.1e-4 / 1.4e-4


def test_dense_sweeps_one_row_per_lane():
    """tiago in the many-body layout (policy 2): 16 friction-loss rows, bounded on both sides, and 2 joint limits — at most 64 rows, one
    per lane.  8 envs at different phases of the fixture's command, two states each."""
    lib = ms.capi.load()
    lib.mjh_set_layout_policy(2)
    try:
        rec, handed = _robot_states("tiago", 8, lambda e: e.dense_solver() == 1)
    finally:
        lib.mjh_set_layout_policy(0)
    assert rec[:, 0].max() <= 64
    _assert_form("dense K = 1 (tiago, friction loss + limits)", rec, handed)
    # measured (MI355X): 16 of 16 instances, 18 rows, 5000 sweeps: median 6.5e-5, 99 % 1.5e-4, max 1.5e-4


def _robot_states(name, nenv, is_form, marks=(40, 50)):
    """a robot fixture alone: env i runs the fixture's command 11 i steps ahead of env 0; the states in front of steps `marks`"""
    ms_, z = _robot(name); mo, _ = _robot(name); m, _ = _robot(name)
    es = ms.Engine(ms_, nenv); e = ms.Engine(_lifted(m), nenv)
    assert is_form(e)
    mo.c.opt.iterations = 1
    for x in (es, e):
        x.set_controlled_dofs(z["controlled"].astype(np.int32))
    es.set_state(qvel=np.tile(z["qvel0"], (nenv, 1)))
    d = orc.OrcData(mo.ptr); d.ifield("controlled")[:] = z["controlled"]
    cmd = lambda k: np.array([robot_command(ms_, k + 11 * i) for i in range(nenv)])
    samples = []
    for k in range(1, marks[-1] + 1):
        if k in marks:
            samples.append(Sample(es, cmd(k), True).reference(d, mo))
        es.set_cmd(ddq=cmd(k)); es.step(1, True)
    out = _device(e, samples)
    es.close(); e.close()
    return out


def test_block_solver_on_the_dense_instances(monkeypatch):
    """pgs_many_body with the list schedule on the QPs of the dense test (MJH_DENSE=0), and the envs beyond a dense capacity of 64 rows
    falling back to it inside the dense chain (MJH_DENSE_CAP=64); both forms' errors side by side per row class"""
    dense, _ = _c4_form("dense", monkeypatch)
    block, handed = _c4_form("block", monkeypatch)
    cap64, handed64 = _c4_form("cap64", monkeypatch)
    for (c, a), b, k in zip(_by_class(dense).items(), _by_class(block).values(), _by_class(cap64).values()):
        print(_line(f"{c[0]}-{c[1]} rows, dense", a)); print(_line(f"{c[0]}-{c[1]} rows, block", b)); print(_line(f"{c[0]}-{c[1]} rows, block behind MJH_DENSE_CAP=64", k))
    _assert_form("block solver, list schedule (C4, MJH_DENSE=0)", block, handed, 193)
    assert cap64[:, 0].min() > 64, "every instance exceeds the capacity"
    _assert_form("block solver as the dense chain's fall-back (C4, MJH_DENSE_CAP=64)", cap64, handed64, 193)
    # measured (MI355X, 5000 sweeps): both runs 38 of 38 instances, 107 .. 216 rows, median 1.0e-5, 99 % 5.6e-5, max 7.6e-5 (equal to the last digit: the same
    # sweeps behind either switch); by class, block against dense, median 1.1e-5 / 3.0e-5, 8.9e-6 / 1.5e-5, 9.8e-6 / 1.3e-5, max 1.7e-5 / 5.9e-5, 2.2e-5 / 5.4e-5, 7.6e-5 / 1.4e-4


def test_lds_resident_articulated_sweeps():
    """layout policy 1, the block sweeps over pools in LDS with general M: tiago (nv 35), pr2 (nv 49) and hsrb4s (nv 32); equality,
    friction-loss and limit rows.  4 envs each, three states each; every robot has its own line and its own floor of 8 instances."""
    lib = ms.capi.load()
    lib.mjh_set_layout_policy(1)
    recs = []; total = 0
    try:
        for name in ("tiago", "pr2", "hsrb4s"):
            rec, handed = _robot_states(name, 4, lambda e: e.dense_solver() == 0 and e.lds_bytes <= 160 * 1024, marks=(40, 50, 60))
            _assert_form(f"LDS-resident {name}", rec, handed)
            recs.append(rec); total += handed
    finally:
        lib.mjh_set_layout_policy(0)
    _assert_form("LDS-resident articulated (tiago, pr2, hsrb4s)", np.concatenate(recs), total)
    # measured (MI355X): 36 of 36 instances, 8 .. 18 rows, 5000 sweeps: median 1.6e-5, 99 % 1.3e-4, max 1.3e-4 (median / max: tiago 6.5e-5 / 1.3e-4, pr2 1.4e-5 / 2.4e-5, hsrb4s 8.9e-6 / 2.3e-5; 12 of 12 each)


# ---------------------------------------------------------------- free bodies: the block forms, the patch sweep
def _free_body_states(make_model, q0_of, nenv, marks, v0_of=None, policy=0, behind=None):
    """a free-body scene from per-env start poses; the states in front of steps `marks` — or, with `behind`, ONE state in which env i
    is behind behind[i] steps"""
    lib = ms.capi.load()
    lib.mjh_set_layout_policy(policy)
    try:
        ms_, mo, m = make_model(), make_model(), _lifted(make_model())
        es = ms.Engine(ms_, nenv); e = ms.Engine(m, nenv)
    finally:
        lib.mjh_set_layout_policy(0)
    mo.c.opt.iterations = 1
    rng = np.random.default_rng(2024)
    q0 = np.array([q0_of(ms_, rng) for _ in range(nenv)])
    es.set_initial_qpos(q0); es.reset()
    if v0_of is not None:
        es.set_state(qvel=np.array([v0_of(ms_, rng) for _ in range(nenv)]))
    d = orc.OrcData(mo.ptr)
    samples = []
    if behind is None:
        done = 0
        for k in marks:
            es.step(k - done); done = k
            samples.append(Sample(es).reference(d, mo))
    else:
        s = None
        for k in range(max(behind) + 1):
            now = Sample(es)
            s = s or now
            for i in range(nenv):
                if behind[i] == k:
                    s.t[i], s.q[i], s.v[i], s.w[i] = now.t[i], now.q[i], now.v[i], now.w[i]
            es.step(1)
        samples.append(s.reference(d, mo))
    es.close()
    return e, samples


def _boxpile_q0(n, shrink, z_of, tilt, seed):
    def q0_of(m, rng):
        q0 = m.array("qpos0").copy()
        r = np.random.default_rng(seed)                       # (the start poses of test_gpu_parity.py's test of this pile)
        for k in range(n):
            q0[7 * k:7 * k + 2] *= shrink; q0[7 * k + 2] = z_of(k)
            quat = r.normal(size=4) * tilt + np.array([1, 0, 0, 0]); q0[7 * k + 3:7 * k + 7] = quat / np.linalg.norm(quat)
        return _yawed(q0, n, rng, 0.15)
    return q0_of


def test_single_block_sweep_of_a_small_pile():
    """boxpile 8, nv 48, pools in LDS (policy 1): the full-wave single-block sweep, NROW = 4"""
    e, samples = _free_body_states(lambda: ms.scene("boxpile", 8), _boxpile_q0(8, 0.55, lambda k: 0.12 + 0.22 * (k // 4) + 0.01 * k, 0.15, 7),
                                   8, (40, 100), policy=1)
    assert e.solver_order() == 2 and e.patch_sweep() == 0 and e.dense_solver() == 0
    rec, handed = _device(e, samples); e.close()
    _assert_form("single-block sweep, NROW = 4 (boxpile 8)", rec, handed)
    # measured (MI355X): 16 of 16 instances, 76 .. 162 rows, 5000 sweeps: median 3.5e-6, 99 % 1.9e-5, max 2.1e-5


def test_lds_resident_acceleration_sweep_of_a_pile():
    """boxpile 16, nv 96, maxcon 96: the running acceleration in LDS, every block gathers / scatters its dofs (NROW = 8)"""
    def model():
        m = ms.scene("boxpile", 16); m.c.maxcon = 96; m.c.maxefc = 96 * 4
        return m
    e, samples = _free_body_states(model, _boxpile_q0(16, 0.55, lambda k: 0.12 + 0.22 * (k // 8) + 0.005 * k, 0.12, 11), 8, (40, 100))
    assert e.solver_order() == 2 and e.patch_sweep() == 0 and e.lds_bytes <= 160 * 1024
    rec, handed = _device(e, samples); e.close()
    _assert_form("LDS-resident acceleration, NROW = 8 (boxpile 16)", rec, handed)
    # measured (MI355X): 16 of 16 instances, 160 .. 304 rows, 5000 sweeps: median 3.4e-6, 99 % 2.5e-5, max 2.8e-5


def test_quad_sweep_with_equality_rows():
    """the pile with <connect> equalities of test_gpu_round3.py: nv 120, more than 64 blocks, single-row blocks (f free) in front of the
    contact blocks.  Per-env start velocities; the boxes no <connect> ties are turned per env as well."""
    from test_gpu_round3 import _pile_with_connects
    lib = ms.capi.load()
    e, samples = _free_body_states(lambda: _pile_with_connects(lib), lambda m, rng: _yawed(m.array("qpos0").copy(), 20, rng, 0.15, first=8), 8, (100, 130),
                                   v0_of=lambda m, rng: rng.normal(size=m.nv) * 0.2)
    assert e.solver_order() == 2 and e.patch_sweep() == 0
    rec, handed = _device(e, samples); e.close()
    assert any(r[0] + 12 > 64 for s in samples for r in s.ref if r is not None), "more than 64 blocks: the grouped order and the quad sweep"
    _assert_form("quad sweep, single-row equality blocks (pile with connects)", rec, handed, 200)
    # measured (MI355X): 16 of 16 instances, 414 .. 444 rows, 5000 sweeps: median 1.7e-4, 99 % 1.9e-3, max 1.9e-3


def test_list_schedule_over_global_pools():
    """boxpile 64 (C2's model), maxcon 600: pgs_many_body with the list schedule over per-env global pools; 8 envs behind 12 .. 30 steps
    of the lattice's collapse, 196 to 1518 rows"""
    def model():
        m = ms.scene("boxpile", 64); m.c.maxcon = 600; m.c.maxefc = 2400
        return m
    behind = [12 + (18 * i) // 7 for i in range(8)]
    e, samples = _free_body_states(model, _boxpile_q0(64, 0.62, lambda k: 0.095 + 0.19 * (k // 16) + 0.002 * (k % 16), 0.05, 5), 8, None, behind=behind)
    assert e.solver_order() == 2 and e.patch_sweep() == 0 and e.dense_solver() == 0
    rec, handed = _device(e, samples); e.close()
    _assert_form("list schedule over global pools (boxpile 64)", rec, handed, 400)
    # measured (MI355X): 8 of 8 instances, 196 .. 1518 rows, 5000 sweeps: median 3.5e-6, 99 % 6.8e-6, max 6.9e-6


def test_fused_patch_sweep():
    """S24 through the fused kernel's contact-patch sweep (csrc/patch_pgs.h; the window solver off): 32 envs behind 300 steps"""
    lib = ms.capi.load()
    ms_, mo, m = ms.scene("s24"), ms.scene("s24"), _lifted(ms.scene("s24"))
    lib.mjh_set_window_solver(0)
    try:
        es = ms.Engine(ms_, 32); e = ms.Engine(m, 32)
    finally:
        lib.mjh_set_window_solver(1)
    assert e.window_solver() == 0 and e.patch_sweep() == 1
    mo.c.opt.iterations = 1
    tab = es.load_s24(); e.load_s24()
    es.step(300)
    s = Sample(es)
    for i in range(32):
        d = oracle_s24(mo, tab, i)
        s.rows(d, i); s.certify(d, mo, i)
    es.close()
    rec, handed = _device(e, [s]); e.close()
    _assert_form("fused patch sweep (S24)", rec, handed)
    # measured (MI355X): 31 of 32 instances, 40 .. 92 rows, 5000 sweeps: median 7.4e-5, 99 % 1.2e-3, max 1.2e-3


@pytest.mark.parametrize("condim", [3, 4])
def test_patch_sweep_with_six_row_contacts(condim):
    """the slab carrying four boxes of test_gpu_fuzz.py: 8 - 10 patches on one body; at condim 4 every contact has six rows (has_dim4)"""
    from test_gpu_fuzz import _table_scene
    lib = ms.capi.load()
    e, samples = _free_body_states(lambda: _table_scene(lib, condim), lambda m, rng: _yawed(m.array("qpos0").copy(), 5, rng, 0.15, first=1), 8, (40, 120))
    assert e.solver_order() == 2 and e.patch_sweep() == 1
    rec, handed = _device(e, samples); e.close()
    _assert_form(f"patch sweep, slab with four boxes, condim {condim}", rec, handed, 16 * (6 if condim == 4 else 4))
    # measured (MI355X): condim 3: 16 of 16 instances, 80 rows, median 4.2e-5, 99 % 6.3e-5, max 6.4e-5; condim 4: 16 of 16, 120 rows, 4.4e-5 / 5.7e-5 / 5.7e-5 (5000 sweeps)
