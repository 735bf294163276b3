"""CPU tests of tests/qp_ref.py, the certified fp64 optimum the GPU tests of test_gpu_qp_forms.py compare every solver form with: the
certificate is reached on constraint programs with every row kind the robots and piles bring (equality, friction loss, joint limit,
pyramidal contact), an independent plain PGS and — where it converges — scipy's L-BFGS-B land on the same point, and defects of the
kind a kernel could have, planted into the program, move qacc beyond the bound the GPU tests assert (so that bound has teeth)."""
import os

import numpy as np
import pytest

import mujoco_sim_amd as ms
import orc
import qp_ref
from conftest import ROOT
from helpers import load_model_tables, oracle_s24
from test_robot_fixtures import robot_command

GPU_BOUND = 1e-2          # what test_gpu_qp_forms.py asserts for the worst instance of a form


class Instance:
    def __init__(self, name, d, m):
        self.name, self.d, self.m = name, d, m
        self.AR, self.b, self.J, self.lo, self.hi = qp_ref.assemble(d, m)
        self.typ = d.ifield("efc_type")[:len(self.b)].copy()
        self.R = d.f("efc_R")[:len(self.b)].copy()
        self.f, self.res = qp_ref.solve(self.AR, self.b, self.lo, self.hi)
        self.qacc = qp_ref.qacc_of(d, self.J, self.f)

    def err(self, f):
        return qp_ref.rel_err(qp_ref.qacc_of(self.d, self.J, f), self.qacc)


def _robot_instance(name, step):
    """the oracle along the fixture's own rollout (test_robot_fixtures.py), the program of step `step`"""
    m, z = load_model_tables(os.path.join(ROOT, "tests", "golden", f"robot_{name}.npz"))
    d = orc.OrcData(m.ptr); d.ifield("controlled")[:] = z["controlled"]
    d.f("qvel")[:] = z["qvel0"]
    for k in range(1, step + 1):
        d.f("ddq")[:] = robot_command(m, k); d.step(1, 1)
    return Instance(f"{name} step {step}", d, m)


def _pile_instance(lib):
    from test_gpu_round3 import _pile_with_connects
    m = _pile_with_connects(lib)
    d = orc.OrcData(m.ptr)
    d.f("qvel")[:] = np.random.default_rng(5).normal(size=m.nv) * 0.2
    d.step(100)                                                  # (dt 0.002: the boxes land after ~40 steps)
    return Instance("pile with connects step 100", d, m)


def _s24_instance():
    m = ms.scene("s24")
    tab = m.s24_randomize(0, 4)
    d = oracle_s24(m, tab, 3)
    d.step(300)
    return Instance("s24 env 3 step 300", d, m)


@pytest.fixture(scope="module")
def instances(lib):
    out = {"c4_30": _robot_instance("c4_pr2_world_objects_mesh", 30), "c4_60": _robot_instance("c4_pr2_world_objects_mesh", 60),
           "pr2_world": _robot_instance("pr2_world", 40), "tiago": _robot_instance("tiago", 40), "pile": _pile_instance(lib),
           "s24": _s24_instance()}
    return out


ROWS = {"c4_30": (151, {0: 6, 3: 1, 6: 144}), "c4_60": (229, {0: 6, 3: 1, 6: 222}), "pr2_world": (104, {0: 6, 3: 2, 6: 96}),
        "tiago": (18, {1: 16, 3: 2})}


def test_the_certificate_is_reached_on_every_row_kind(instances):
    for key, s in instances.items():
        n = len(s.b)
        kinds = {int(t): int((s.typ == t).sum()) for t in np.unique(s.typ)}
        print(f"QP-REF {s.name}: {n} rows {kinds}, cond(AR) {np.linalg.cond(s.AR):.1e}, KKT residual {s.res:.1e}, max|b| {np.abs(s.b).max():.0f}, "
              f"rows at a bound {int(((s.f <= s.lo) | (s.f >= s.hi)).sum())}")
        if key in ROWS:
            assert (n, kinds) == ROWS[key], s.name
        assert qp_ref.certified(s.AR, s.b, s.res), (s.name, s.res)
        assert (s.f >= s.lo).all() and (s.f <= s.hi).all()
    p = instances["pile"]
    assert (p.typ == qp_ref.EQUALITY).sum() == 12 and (p.typ == 6).sum() >= 200, "four <connect>s and a landed pile"
    # two-sided rows both ways: friction-loss rows saturated at a limit, others strictly inside, some of them pulling the negative way
    t = instances["tiago"]; fr = t.typ == qp_ref.FRICTION_DOF
    at = (t.f[fr] <= t.lo[fr]) | (t.f[fr] >= t.hi[fr])
    assert at.any() and (~at & (t.f[fr] < 0)).any() and (~at & (t.f[fr] > 0)).any()


def test_a_poor_guess_reaches_the_same_certified_point(instances):
    """the certificate, not the guess, makes the optimum: from zero and from the oracle's own single-sweep forces"""
    for s in instances.values():
        for guess in (np.zeros(len(s.b)), s.d.f("efc_force")[:len(s.b)].copy()):
            f, res = qp_ref.solve(s.AR, s.b, s.lo, s.hi, guess=guess)
            assert qp_ref.certified(s.AR, s.b, res), (s.name, res)
            assert s.err(f) <= 1e-10, s.name


def test_an_independent_fp64_pgs_lands_on_the_certified_optimum(instances):
    for s in instances.values():
        f = qp_ref.pgs(s.AR, s.b, s.lo, s.hi, 3000)
        e = s.err(f)
        print(f"QP-REF {s.name}: numpy fp64 PGS, 3000 sweeps from zero: qacc {e:.1e}")
        assert e <= 1e-10, s.name


def test_lbfgsb_agrees_where_it_converges(instances):
    """scipy's L-BFGS-B with the options of the former reference of test_gpu_round5.py, kept where it passes that test's filter
    (KKT residual <= 1e-6 max(1, |b|)).  Its distance from the optimum is then bounded: with rho the vector of KKT violations of a
    feasible f and f* the optimum,  lmin |f - f*|^2 <= (f - f*)' AR (f - f*) = (g - g*)'(f - f*) <= |rho| |f - f*|  (the
    optimality conditions of f* make g*'(f - f*) >= 0, and the components of g that rho leaves out have the sign that makes
    g'(f* - f) >= 0), so |f - f*| <= |rho| / lmin(AR) with |rho| <= sqrt(n) kkt, and  |qacc - qacc*| <= |M^-1 J'|_2 |f - f*|; also
    dq'M dq = df'(J M^-1 J')df <= df'AR df <= |rho|^2 / lmin(AR), so |dq| <= |rho| / sqrt(lmin(AR) lmin(M)).  The smaller of the two is
    asserted; both are worst-case bounds (the smallest eigenvalue of AR is R's scale), the measured distance is printed."""
    from scipy.optimize import minimize
    passed = []
    for key, s in instances.items():
        n = len(s.b)
        res = minimize(lambda x: 0.5 * x @ s.AR @ x + s.b @ x, np.zeros(n), jac=lambda x: s.AR @ x + s.b,
                       bounds=[(None if l == -np.inf else l, None if h == np.inf else h) for l, h in zip(s.lo, s.hi)],
                       method="L-BFGS-B", options=dict(maxiter=50000, maxfun=200000, ftol=1e-18, gtol=1e-13))
        f = np.clip(res.x, s.lo, s.hi)
        k = qp_ref.kkt(s.AR, s.b, s.lo, s.hi, f)
        ok = k <= 1e-6 * max(1.0, np.abs(s.b).max())
        e = s.err(f)
        MiJt = np.array([s.d.solve_m(s.J[i]) for i in range(n)]).T
        nv = s.J.shape[1]
        M = np.array([s.d.mul_m(np.eye(nv)[q]) for q in range(nv)])
        rho, lmin = np.sqrt(n) * k, np.linalg.eigvalsh(s.AR)[0]
        bound = min(np.linalg.norm(MiJt, 2) * rho / lmin, rho / np.sqrt(lmin * np.linalg.eigvalsh(M)[0])) / max(1.0, np.abs(s.qacc).max())
        print(f"QP-REF {s.name}: L-BFGS-B KKT residual {k:.1e} ({'passes' if ok else 'fails'} the 1e-6 filter), qacc {e:.1e} (bound from its residual {bound:.1e})")
        if ok:
            passed.append(key)
            assert e <= bound, s.name
    assert "s24" in passed


def _active(s, mask):
    """rows of `mask` that carry force in the optimum, strongest first"""
    idx = np.nonzero(mask & (s.f != 0) & ~((s.f <= s.lo) | (s.f >= s.hi)))[0]
    return idx[np.argsort(-np.abs(s.f[idx]))]


def test_planted_defects_move_qacc_beyond_the_gpu_bound(instances):
    """what a kernel could get wrong, planted into the program of an instance at rows that are active in its optimum; the defective
    program solved the same way (the zeroed tile leaves no symmetric matrix and no QP: there, 300 sweeps of the plain PGS from the
    optimum, which is what such a kernel would run)"""
    found = {}
    # a friction-loss row clamped at f >= 0 (its lower bound lost): tiago, the free friction row that pulls hardest the negative way
    t = instances["tiago"]
    i = [k for k in _active(t, t.typ == qp_ref.FRICTION_DOF) if t.f[k] < 0][0]
    lo = t.lo.copy(); lo[i] = 0.0
    found["friction-loss row at f >= 0"] = (t, t.err(qp_ref.solve(t.AR, t.b, lo, t.hi)[0]))
    # an equality row clamped at f >= 0: a joint equality of the PR2, a <connect> row of the pile
    for key in ("pr2_world", "pile"):
        s = instances[key]
        i = [k for k in _active(s, s.typ == qp_ref.EQUALITY) if s.f[k] < 0][0]
        lo = s.lo.copy(); lo[i] = 0.0
        found[f"equality row {i} at f >= 0 ({key})"] = (s, s.err(qp_ref.solve(s.AR, s.b, lo, s.hi)[0]))
    # one off-diagonal 16 x 16 tile of AR zeroed: the tile whose product with the optimum is largest
    s = instances["c4_60"]; n = len(s.b); nt = (n + 15) // 16
    best = max(((np.abs(s.AR[16 * a:16 * a + 16, 16 * c:16 * c + 16] @ s.f[16 * c:16 * c + 16]).max(), a, c)
                for a in range(nt) for c in range(nt) if a != c))
    A = s.AR.copy(); A[16 * best[1]:16 * best[1] + 16, 16 * best[2]:16 * best[2] + 16] = 0.0
    f = qp_ref.pgs(A, s.b, s.lo, s.hi, 300, f0=s.f)
    found[f"AR tile ({best[1]}, {best[2]}) zeroed"] = (s, s.err(f))
    # R left out of one diagonal entry: the active row with the largest R f
    s = instances["pr2_world"]
    act = (s.f > s.lo) & (s.f < s.hi)
    i = int(np.argmax(np.where(act, s.R * np.abs(s.f), 0.0)))
    A = s.AR.copy(); A[i, i] -= s.R[i]
    found[f"R missing on the diagonal of row {i}"] = (s, s.err(qp_ref.solve(A, s.b, s.lo, s.hi)[0]))
    for what, (s, e) in found.items():
        print(f"QP-REF planted in {s.name}: {what}: qacc moves {e:.1e}")
    for what, (s, e) in found.items():
        assert e > GPU_BOUND, (what, s.name, e)


def test_fp32_yardstick(instances):
    """what single precision alone costs on these programs: from the certified optimum rounded to float32, 200 float32 sweeps on AR
    formed in float32 from rounded J, M^-1 and R.  A yardstick to read the device's figures against, not a bound for them: the
    device also computes kinematics, J and M^-1 in fp32."""
    for s in instances.values():
        n, nv = s.J.shape
        Minv = np.array([s.d.solve_m(np.eye(nv)[k]) for k in range(nv)]).astype(np.float32)
        J = s.J.astype(np.float32)
        AR = J @ (Minv @ J.T) + np.diag(s.R.astype(np.float32))
        rel = np.abs(AR - s.AR).max() / np.abs(s.AR).max()
        f = qp_ref.pgs(AR, s.b, s.lo, s.hi, 200, f0=s.f.astype(np.float32), dtype=np.float32)
        e = s.err(f.astype(np.float64))
        print(f"QP-REF {s.name}: fp32 yardstick: AR formed in float32 differs by {rel:.1e}, 200 float32 sweeps from the optimum: qacc {e:.1e}")
        assert e < 1e-4, s.name
