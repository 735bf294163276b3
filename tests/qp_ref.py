"""Certified fp64 optimum of a step's constraint program.  Test infrastructure only (numpy; no PGS of the oracle takes part).

The constrained accelerations of a step solve   min 1/2 f'AR f + b'f,  lo <= f <= hi   with AR = J M^-1 J' + R, R > 0: strictly convex,
so the optimum is unique whatever the order, schedule or storage of a solver's sweeps.  `assemble` reads the program from an oracle
that has just stepped, `solve` finds its optimum by a primal active-set iteration with exact solves of the free rows, and the KKT
residual it returns is the certificate: an instance counts only where  residual <= CERT * max(1, max|b|)."""
import numpy as np

EQUALITY, FRICTION_DOF = 0, 1          # MJH_CNSTR_* (include/mjhip.h); every other kind is one-sided
CERT = 1e-10


def assemble(d, m):
    """(AR, b, J, lo, hi) of the step an OrcData has just taken (d.step(1, with_inverse) with opt.iterations = 1: the assembly is that
    of the pre-step state, the oracle's single sweep is not used)."""
    n = d.i("nefc"); nv = m.nv
    AR = d.f("efc_AR")[:n * n].reshape(n, n).copy(); b = d.f("efc_b")[:n].copy(); J = d.f("efc_J")[:n * nv].reshape(n, nv).copy()
    typ = d.ifield("efc_type")[:n]; idx = d.ifield("efc_id")[:n]
    lo = np.zeros(n); hi = np.full(n, np.inf)
    lo[typ == EQUALITY] = -np.inf
    fr = typ == FRICTION_DOF
    if fr.any():
        fl = np.asarray(m.array("dof_frictionloss"), dtype=np.float64)[idx[fr]]
        lo[fr] = -fl; hi[fr] = fl
    return AR, b, J, lo, hi


def kkt(AR, b, lo, hi, f):
    """largest violation of the optimality conditions: |g| on free rows, max(-g, 0) at a lower bound, max(g, 0) at an upper bound"""
    g = AR @ f + b
    at_lo = f <= lo; at_hi = f >= hi
    r = np.where(at_lo & at_hi, 0.0, np.where(at_lo, np.maximum(-g, 0.0), np.where(at_hi, np.maximum(g, 0.0), np.abs(g))))
    return float(r.max(initial=0.0))


def pgs(AR, b, lo, hi, sweeps, f0=None, dtype=np.float64):
    """plain projected Gauss-Seidel in natural row order (numpy, in `dtype`): the approximate solution a guess is taken from, and the
    independent solver the reference is compared with"""
    A = np.ascontiguousarray(AR, dtype=dtype); bb = b.astype(dtype); l = lo.astype(dtype); h = hi.astype(dtype)
    f = np.zeros(len(b), dtype=dtype) if f0 is None else np.clip(f0.astype(dtype), l, h)
    dinv = (1 / np.diag(A)).astype(dtype)
    for _ in range(sweeps):
        for i in range(len(bb)):
            x = f[i] - (bb[i] + A[i] @ f) * dinv[i]
            f[i] = l[i] if x < l[i] else (h[i] if x > h[i] else x)
    return f


def solve(AR, b, lo, hi, guess=None, maxiter=None):
    """-> (f, KKT residual).  Primal active set: the free set of the guess, exact solve of the free rows, step to the first bound on
    the way there; at a stationary point the bound rows whose multiplier has the wrong sign are released (all of them at first, one
    at a time — the textbook rule, which cannot cycle — once that has not ended the iteration)."""
    n = len(b)
    if guess is None:
        guess = pgs(AR, b, lo, hi, 100)
    f = np.clip(np.asarray(guess, dtype=np.float64), lo, hi)
    bound = (f <= lo) | (f >= hi)
    maxiter = maxiter or 20 * n + 100
    for it in range(maxiter):
        F = ~bound
        x = f.copy()
        if F.any():
            x[F] = np.linalg.solve(AR[np.ix_(F, F)], -(b[F] + AR[np.ix_(F, bound)] @ f[bound]))
        p = x - f
        with np.errstate(divide="ignore", invalid="ignore"):
            a = np.where(p < 0, (lo - f) / p, np.where(p > 0, (hi - f) / p, np.inf))
        a[bound] = np.inf
        k = int(np.argmin(a)) if n else 0
        if n and a[k] < 1.0:                                   # blocked: stop at the first bound met, that row joins the bound set
            f = f + a[k] * p
            f[k] = lo[k] if p[k] < 0 else hi[k]
            bound[k] = True
            continue
        f = x
        g = AR @ f + b
        wrong = bound & (((f <= lo) & (g < 0)) | ((f >= hi) & (g > 0)))
        wrong &= np.abs(g) > CERT * 1e-2 * max(1.0, np.abs(b).max(initial=0.0))
        if not wrong.any():
            break
        if it < n:
            bound[wrong] = False
        else:
            bound[np.argmax(np.where(wrong, np.abs(g), 0.0))] = False
    return f, kkt(AR, b, lo, hi, f)


def certified(AR, b, res):
    return res <= CERT * max(1.0, float(np.abs(b).max(initial=0.0)))


def qacc_of(d, J, f):
    """qacc_smooth + M^-1 J' f"""
    return d.f("qacc_smooth") + d.solve_m(J.T @ f)


def rel_err(qacc, ref):
    """the measure of every comparison with the optimum: max |delta| / max(1, max |ref|)"""
    return float(np.abs(qacc - ref).max() / max(1.0, np.abs(ref).max()))
