"""GPU tests of the lean window instance (csrc/window.hip: mjh_window_kernel<24, 6, true, 2, 1>, what S24's launches without the LDS
tier run so that an assemble wavefront fits on the window wavefront's SIMD): envs beyond 128 rows — the third 64-row window, which the
lean instance keeps in LDS instead of registers, and the 16-row form's windows beyond the register-resident ones — are swept to the
same values whichever instance runs.

Scene: S24's pen and boxes released flat 2 x 2 (bench.py's S24D layout) with a contact capacity of 64 and the window capacity lowered
to 16 windows = 256 rows (MJH_WINDOW_MAXW, the tests' knob): the model class of S24 (rows within 256, 64-row form for 97 .. 192 rows,
the instance chosen by the rows the cohort has seen), but with envs of 129 .. 256 rows after the boxes have landed (an env whose
rows exceed 256 drops whole blocks behind them and raises the capacity flag: deterministic, and left out of the oracle check)."""
import numpy as np
import pytest

import mujoco_sim_amd as ms
from helpers import oracle_s24

pytestmark = pytest.mark.gpu

PEN, CAPACITY, MAXW = 0.175, 64, 16


def _engine(nenv, lean, monkeypatch):
    """bench.py's S24D release for env ids 0 .. nenv - 1 at the small capacity; lean: 1 / 0 force the lean / the fat instance, None: the engine's own choice"""
    m = ms.scene("s24pen", PEN, CAPACITY)
    if lean is None:
        monkeypatch.delenv("MJH_WINDOW_LEAN", raising=False)
    else:
        monkeypatch.setenv("MJH_WINDOW_LEAN", str(lean))
    monkeypatch.setenv("MJH_WINDOW_MAXW", str(MAXW))
    e = ms.Engine(m, nenv)
    monkeypatch.delenv("MJH_WINDOW_LEAN", raising=False); monkeypatch.delenv("MJH_WINDOW_MAXW")
    assert e.window_solver() == 1
    parts = [m.s24_randomize(int(s), 1) for s in range(nenv)]
    tab = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    q = tab["qpos"].reshape(nenv, 4, 7)
    for i in range(nenv):
        rng = np.random.default_rng(0x524D0000 + i)
        for k in range(4):
            yaw = rng.uniform(-0.3, 0.3)
            q[i, k] = [(-1 if k & 1 else 1) * PEN / 2, (-1 if k & 2 else 1) * PEN / 2, 0.16 + 0.02 * k, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
    e.load_tables(tab)
    return m, e, tab


def test_envs_beyond_128_rows_are_swept_alike_by_the_lean_and_the_fat_window_instance(monkeypatch):
    """Three things about the envs beyond 128 rows of a model within 256 rows:
    (1) forced lean, forced fat and the engine's own choice of instance leave identical states and statistics after 150 steps from
        release, and two runs of the lean instance are identical;
    (2) the run contains such envs in both forms: 129 .. 192 rows (64-row form: third window in LDS in the lean instance, in
        registers in the fat one) and beyond 192 (16-row form: windows 7 .. streamed from the env's global slice in the lean
        instance, from the LDS tier in the fat one);
    (3) those envs, stepped once by the lean instance from its own state, match the fp64 oracle within the tolerances the window-form
        tests use (tests/test_gpu_teacher_forced.py: S24_TOL_Q = 1e-6, S24_TOL_V = 2e-5, relative to max(1, |x|))."""
    from test_gpu_teacher_forced import S24_TOL_Q, S24_TOL_V
    nenv, nsteps = 1536, 150          # (>= 1024 envs: the engine keeps the cohorts' largest row counts and chooses the instance by them)
    outs = {}
    seen129 = seen193 = 0
    for name, lean in (("lean", 1), ("fat", 0), ("auto", None), ("lean2", 1)):
        m, e, tab = _engine(nenv, lean, monkeypatch)
        if name == "lean":
            # row counts along the way (one step at a time): both classes must occur
            for _ in range(nsteps):
                e.step(1)
                r = e.get_stats()[:, 1]
                seen129 += int(((r > 128) & (r <= 192)).sum()); seen193 += int((r > 192).sum())
        else:
            for _ in range(nsteps):
                e.step(1)
        e.synchronize()
        t, q, v, w = e.get_state(); st = e.get_stats()
        outs[name] = (t.copy(), q.copy(), v.copy(), w.copy(), st[:, :3].copy(), (st[:, 3] & 0xff).copy())
        if name != "lean":
            e.close()
        else:
            lean_engine, lean_tab, lean_model = e, tab, m
    print(f"WINDOW-LEAN: env-steps with 129 .. 192 rows: {seen129}, beyond 192: {seen193} of {nenv * nsteps}")
    assert seen129 >= 1000 and seen193 >= 100, "the run must contain envs beyond 128 rows in both forms"
    for other in ("fat", "auto", "lean2"):
        for k, (x, y) in enumerate(zip(outs["lean"], outs[other])):
            assert np.array_equal(x, y), f"lean against {other}: array {k} differs in {int((x != y).any(axis=-1).sum() if x.ndim > 1 else (x != y).sum())} envs"
    # (3) one step of the lean instance against the oracle, envs beyond 128 rows
    e = lean_engine
    t, q, v, w = e.get_state()
    e.step(1); e.synchronize()
    _, q1, v1, _ = e.get_state(); st = e.get_stats()
    rows = st[:, 1]
    ok = (st[:, 3] & 7) == 0
    pick = np.concatenate([np.nonzero(ok & (rows > 128) & (rows <= 192))[0][:16], np.nonzero(ok & (rows > 192))[0][:16]])
    assert (rows[pick] <= 192).sum() >= 8 and (rows[pick] > 192).sum() >= 4, "envs of both forms without a capacity flag"
    checked = {"64-row": 0, "16-row": 0}
    worst_q = worst_v = 0.0
    for i in pick:
        d = oracle_s24(lean_model, lean_tab, int(i))
        d.f("qpos")[:] = q[i]; d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = w[i]; d.f("qacc")[:] = w[i]; d.f("time")[0] = t[i]
        d.step(1)
        if d.i("ncon") != st[i, 0] or d.i("nefc") != st[i, 1]:
            continue          # (a contact at the margin seen by one side only: not the same problem)
        eq = float(np.abs(q1[i] - d.f("qpos")).max() / max(1, np.abs(d.f("qpos")).max()))
        ev = float(np.abs(v1[i] - d.f("qvel")).max() / max(1, np.abs(d.f("qvel")).max()))
        worst_q = max(worst_q, eq); worst_v = max(worst_v, ev)
        checked["64-row" if rows[i] <= 192 else "16-row"] += 1
        print(f"WINDOW-LEAN vs oracle: env {int(i)} rows {int(rows[i])} sweeps {int(st[i, 2])}: qpos {eq:.2e} qvel {ev:.2e}")
    print(f"WINDOW-LEAN vs oracle: checked {checked}, worst qpos {worst_q:.2e} qvel {worst_v:.2e}")
    assert checked["64-row"] >= 6 and checked["16-row"] >= 3
    assert worst_q <= S24_TOL_Q and worst_v <= S24_TOL_V
    e.close()


def test_s24_states_do_not_depend_on_the_window_instance(monkeypatch):
    """S24 itself, 2048 envs from release through the landing of the boxes (300 steps): the lean instance, the fat one and the engine's
    own choice (fat until the cohorts' row counts are known and while an env is beyond 128 rows, lean otherwise) are bitwise equal."""
    m = ms.scene("s24")
    outs = []
    for lean in (1, 0, None):
        if lean is None:
            monkeypatch.delenv("MJH_WINDOW_LEAN", raising=False)
        else:
            monkeypatch.setenv("MJH_WINDOW_LEAN", str(lean))
        e = ms.Engine(m, 2048)
        monkeypatch.delenv("MJH_WINDOW_LEAN", raising=False)
        e.load_s24(); e.set_cohorts(3)
        rmax = 0
        for _ in range(10):
            e.step(30); rmax = max(rmax, int(e.get_stats()[:, 1].max()))
        t, q, v, w = e.get_state(); st = e.get_stats()
        outs.append((q.copy(), v.copy(), w.copy(), st[:, :3].copy()))
        e.close()
    print(f"S24-LEAN: largest row count at the ten looks: {rmax}")
    for o in outs[1:]:
        for x, y in zip(outs[0], o):
            assert np.array_equal(x, y)
