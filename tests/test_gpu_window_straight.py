"""GPU tests of the lean window instance's straight-line sweep loops (csrc/window_kernel.h: wavefronts of `mjh_window_kernel<24, 6, true, 2, 1>`
whose windows are all register-resident sweep in a loop written out for their number of window pairs; MJH_WINDOW_STRAIGHT=0 keeps them
in the general loop).

Scene: S24's model class in a pen — S24D's pen with a contact capacity of 64 and the window capacity lowered to 16 windows
(MJH_WINDOW_MAXW: a model within 256 rows, so the lean instance may run it; MJH_WINDOW_LEAN=1 forces it — an engine of fewer than
1024 envs does not track its cohorts' row counts).  256 envs in three cohorts, 150 steps.  The envs of the first two cohorts are released
as S24 releases them (four boxes of random size dropped one above the other): the boxes land one after the other, the rows of an env
grow from nothing to at most 96 through every window count (fp64 oracle: 64 such envs stay within 96 rows).  The envs of the third
cohort are released flat 2 x 2 (bench.py's S24D layout): they pass 97 .. 128 rows and settle at 129 .. 192 (oracle, 16 such envs:
1043 / 588 of 2400 env-steps)."""
import numpy as np
import pytest

import mujoco_sim_amd as ms
from helpers import oracle_s24

pytestmark = pytest.mark.gpu

PEN, CAPACITY, MAXW = 0.175, 64, 16
NENV, NCOHORT, NSTEPS = 256, 3, 150
NW = 6                    # register-resident windows of the 16-row form (window_pgs.h: WN_NW24)
ROWS64 = (96, 192)        # envs of 97 .. 192 rows take the 64-row form (WN32_MIN_ROWS, 64 WN64_NW)


def _engine(monkeypatch, straight, win64=None, nenv=NENV, nflat=NENV - NENV * 2 // 3):
    m = ms.scene("s24pen", PEN, CAPACITY)
    monkeypatch.setenv("MJH_WINDOW_LEAN", "1"); monkeypatch.setenv("MJH_WINDOW_MAXW", str(MAXW)); monkeypatch.setenv("MJH_WINDOW_STRAIGHT", str(straight))
    if win64 is not None:
        monkeypatch.setenv("MJH_WINDOW64", str(win64))
    e = ms.Engine(m, nenv)
    for k in ("MJH_WINDOW_LEAN", "MJH_WINDOW_MAXW", "MJH_WINDOW_STRAIGHT", "MJH_WINDOW64"):
        monkeypatch.delenv(k, raising=False)
    assert e.window_solver() == 1
    parts = [m.s24_randomize(int(s), 1) for s in range(nenv)]
    tab = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    q = tab["qpos"].reshape(nenv, 4, 7)
    for i in range(nenv - nflat, nenv):          # the last nflat envs: flat 2 x 2
        rng = np.random.default_rng(0x524D0000 + i)
        for k in range(4):
            yaw = rng.uniform(-0.3, 0.3)
            q[i, k] = [(-1 if k & 1 else 1) * PEN / 2, (-1 if k & 2 else 1) * PEN / 2, 0.16 + 0.02 * k, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
    e.load_tables(tab)
    return m, e, tab


def _run(monkeypatch, straight, win64=None):
    """-> (state, warm start, statistics) after NSTEPS steps, the rows of every env in every step [NSTEPS, NENV], the engine's stats words of the last step"""
    m, e, tab = _engine(monkeypatch, straight, win64)
    e.set_cohorts(NCOHORT)
    rows = np.zeros((NSTEPS, NENV), dtype=np.int64)
    for k in range(NSTEPS):
        e.step(1)
        rows[k] = e.get_stats()[:, 1]
    e.synchronize()
    t, q, v, w = e.get_state(); st = e.get_stats()
    out = (t.copy(), q.copy(), v.copy(), w.copy(), st[:, :3].copy(), (st[:, 3] & 0xff).copy())
    e.close()
    return out, rows, st.copy()


def _wave_windows(rows, form64):
    """largest window count of every wavefront of the 16-row section in every step: four consecutive envs of a cohort's range
    (fewer than 1024 envs: launch order = env order), envs of the 64-row form left out"""
    w = np.where(form64, 0, (rows + 15) // 16)
    out = []
    for g in range(NCOHORT):
        g0, g1 = NENV * g // NCOHORT, NENV * (g + 1) // NCOHORT
        for s in range(g0, g1, 4):
            out.append(w[:, s:min(s + 4, g1)].max(axis=1))
    return np.stack(out, axis=1)


@pytest.fixture(scope="module")
def straight_run():
    mp = pytest.MonkeyPatch()
    try:
        yield _run(mp, 1)
    finally:
        mp.undo()


def test_straight_loops_are_bitwise_the_general_loop(straight_run, monkeypatch):
    """MJH_WINDOW_STRAIGHT=1 against =0 and against a second =1 run: state, warm start and statistics after 150 steps are equal bit for bit;
    the run has wavefronts of every window count 1 .. 6 (each straight-line body, last pair and last odd window) and envs of the 64-row form."""
    out1, rows, _ = straight_run
    form64 = (rows > ROWS64[0]) & (rows <= ROWS64[1])
    nw = _wave_windows(rows, form64)
    counts = np.bincount(nw.ravel(), minlength=NW + 1)
    n64 = int(((rows > 96) & (rows <= 128)).sum())
    print(f"WINDOW-STRAIGHT: wavefront-steps by largest window count 0 .. : {counts.tolist()}; env-steps with 97 .. 128 rows: {n64}, beyond 128: {int((rows > 128).sum())}")
    assert all(counts[k] > 0 for k in range(1, NW + 1)), "wavefronts of every window count 1 .. 6 must occur"
    assert n64 > 0, "some envs must reach 97 .. 128 rows and take the 64-row form"
    for name, straight in (("general", 0), ("straight again", 1)):
        out, rows2, _ = _run(monkeypatch, straight)
        assert np.array_equal(rows, rows2)
        for k, (x, y) in enumerate(zip(out1, out)):
            assert np.array_equal(x, y), f"straight against {name}: array {k} differs"


def test_straight_loops_without_the_64_row_section(monkeypatch):
    """MJH_WINDOW64=0: wavefronts with an env beyond six windows take the general loop, the others the straight ones; bitwise as above"""
    out1, rows, _ = _run(monkeypatch, 1, win64=0)
    beyond = int((rows > 128).sum())        # (97 .. 128 rows: the 32-row form; beyond: the 16-row form's windows 7 ..)
    print(f"WINDOW-STRAIGHT, no 64-row section: env-steps beyond 128 rows: {beyond}")
    assert beyond > 0, "envs beyond six windows in the 16-row form must occur"
    for straight in (0, 1):
        out, rows2, _ = _run(monkeypatch, straight, win64=0)
        assert np.array_equal(rows, rows2)
        for k, (x, y) in enumerate(zip(out1, out)):
            assert np.array_equal(x, y), f"MJH_WINDOW64=0, straight against MJH_WINDOW_STRAIGHT={straight}: array {k} differs"


def test_straight_loops_against_the_oracle(monkeypatch):
    """32 envs (the last eight released flat: beyond 96 rows, the 64-row form), one step from the state after 60 steps against the fp64 oracle, within the bounds of tests/test_gpu_window_lean.py: qpos 1e-6, qvel 2e-5
    (relative to max(1, |x|))"""
    nenv = 32
    m, e, tab = _engine(monkeypatch, 1, nenv=nenv, nflat=8)
    e.step(60); e.synchronize()
    t, q, v, w = e.get_state()
    e.step(1); e.synchronize()
    _, q1, v1, _ = e.get_state(); st = e.get_stats()
    worst_q = worst_v = 0.0
    checked = 0
    for i in range(nenv):
        if st[i, 3] & 7:
            continue      # (capacity flag: rows were dropped, not the same problem)
        d = oracle_s24(m, tab, i)
        d.f("qpos")[:] = q[i]; d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = w[i]; d.f("qacc")[:] = w[i]; d.f("time")[0] = t[i]
        d.step(1)
        if d.i("ncon") != st[i, 0] or d.i("nefc") != st[i, 1]:
            continue      # (a contact at the margin seen by one side only: not the same problem)
        eq = float(np.abs(q1[i] - d.f("qpos")).max() / max(1, np.abs(d.f("qpos")).max()))
        ev = float(np.abs(v1[i] - d.f("qvel")).max() / max(1, np.abs(d.f("qvel")).max()))
        worst_q = max(worst_q, eq); worst_v = max(worst_v, ev); checked += 1
    print(f"WINDOW-STRAIGHT vs oracle: {checked} of {nenv} envs, rows {int(st[:, 1].min())} .. {int(st[:, 1].max())}, worst qpos {worst_q:.2e} qvel {worst_v:.2e}")
    e.close()
    assert checked >= nenv // 2
    assert worst_q <= 1e-6 and worst_v <= 2e-5
