"""GPU tests of the window sweeps without their unneeded wait states (csrc/window_kernel.h; the lane-constant selects stay v_cndmask).
That change moves no value: no operand, no order of any sum, and a select stays a select.  So the state after 150
steps must be, bit for bit, what the library of the commit before it computed on the MI355X: tests/golden/window_slots_hashes.json holds
the SHA-256 of qpos, qvel, qacc_warmstart and the statistics from that library (its commit id and how it was produced are in the file; a
later change that moves rounding on purpose regenerates it with `python tests/test_gpu_window_slots.py OUT.json`).

Scene: the one of tests/test_gpu_window_straight.py — S24's model class in a pen, 256 envs in three cohorts, 150 steps; two cohorts
released as S24 releases them (the rows of an env grow from nothing through every window count), the third flat 2 x 2 (97 .. 128 rows and
beyond: the 64-row form).  Three runs: the defaults of that scene (lean instance, 64-row section on), MJH_WINDOW64=0 (every env in the
16-row / 32-row paths) and MJH_WINDOW_LEAN=0 (the fat instance)."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import mujoco_sim_amd as ms

pytestmark = pytest.mark.gpu

PEN, CAPACITY, MAXW = 0.175, 64, 16
NENV, NCOHORT, NSTEPS = 256, 3, 150
NW = 6                    # register-resident windows of the 16-row form
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_slots_hashes.json")
RUNS = {"default": dict(), "window64_0": dict(win64=0), "lean_0": dict(lean=0)}


def _engine(monkeypatch, lean=1, win64=None, nenv=NENV, nflat=NENV - NENV * 2 // 3):
    m = ms.scene("s24pen", PEN, CAPACITY)
    monkeypatch.setenv("MJH_WINDOW_LEAN", str(lean)); monkeypatch.setenv("MJH_WINDOW_MAXW", str(MAXW))
    if win64 is not None:
        monkeypatch.setenv("MJH_WINDOW64", str(win64))
    e = ms.Engine(m, nenv)
    for k in ("MJH_WINDOW_LEAN", "MJH_WINDOW_MAXW", "MJH_WINDOW64"):
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


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _run(monkeypatch, lean=1, win64=None):
    """-> ({array name: sha256} after NSTEPS steps, the rows of every env in every step [NSTEPS, NENV])"""
    m, e, tab = _engine(monkeypatch, lean, win64)
    e.set_cohorts(NCOHORT)
    rows = np.zeros((NSTEPS, NENV), dtype=np.int64)
    for k in range(NSTEPS):
        e.step(1)
        rows[k] = e.get_stats()[:, 1]
    e.synchronize()
    t, q, v, w = e.get_state(); st = e.get_stats()
    h = {"qpos": _sha(q), "qvel": _sha(v), "qacc_warmstart": _sha(w), "stats": _sha(st[:, :3].astype(np.int32)), "flags": _sha((st[:, 3] & 0xff).astype(np.int32))}
    e.close()
    return h, rows


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
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_state_is_bitwise_the_parents(golden, monkeypatch):
    """(a) the scene's defaults: wavefronts of every window count 1 .. 6 and envs of 97 .. 128 rows occur, and the hashes are the recorded ones"""
    h, rows = _run(monkeypatch)
    form64 = (rows > 96) & (rows <= 192)
    counts = np.bincount(_wave_windows(rows, form64).ravel(), minlength=NW + 1)
    n64 = int(((rows > 96) & (rows <= 128)).sum())
    print(f"WINDOW-SLOTS: wavefront-steps by largest window count 0 .. : {counts.tolist()}; env-steps with 97 .. 128 rows: {n64}; hashes {h}")
    assert all(counts[k] > 0 for k in range(1, NW + 1)), "wavefronts of every window count 1 .. 6 must occur"
    assert n64 > 0, "some envs must reach 97 .. 128 rows and take the 64-row form"
    assert h == golden["hashes"]["default"]


@pytest.mark.parametrize("name", ["window64_0", "lean_0"])
def test_state_is_bitwise_the_parents_other_paths(golden, monkeypatch, name):
    """(b) MJH_WINDOW64=0: every 16-row path (and the 32-row form); MJH_WINDOW_LEAN=0: the fat instance"""
    h, rows = _run(monkeypatch, **RUNS[name])
    print(f"WINDOW-SLOTS {name}: rows up to {int(rows.max())}; hashes {h}")
    assert h == golden["hashes"][name]


def test_one_step_against_the_oracle(monkeypatch):
    """(c) 32 envs (the last eight released flat: beyond 96 rows, the 64-row form), one step from the state after 60 steps against the fp64
    oracle, within the bounds of tests/test_gpu_window_lean.py: qpos 1e-6, qvel 2e-5 (relative to max(1, |x|))"""
    from helpers import oracle_s24
    nenv = 32
    m, e, tab = _engine(monkeypatch, nenv=nenv, nflat=8)
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
    print(f"WINDOW-SLOTS vs oracle: {checked} of {nenv} envs, rows {int(st[:, 1].min())} .. {int(st[:, 1].max())}, worst qpos {worst_q:.2e} qvel {worst_v:.2e}")
    e.close()
    assert checked >= nenv // 2
    assert worst_q <= 1e-6 and worst_v <= 2e-5


if __name__ == "__main__":      # regenerate the recorded hashes with the library in use (MJHIP_LIB selects a build): python tests/test_gpu_window_slots.py OUT.json [commit id]
    mp = pytest.MonkeyPatch()
    out = {"parent_commit": sys.argv[2] if len(sys.argv) > 2 else "",
           "produced_by": "python tests/test_gpu_window_slots.py OUT.json COMMIT, on one MI355X, with the library built from that commit",
           "scene": f"s24pen {PEN} {CAPACITY}, MJH_WINDOW_MAXW={MAXW}, {NENV} envs, {NCOHORT} cohorts, {NSTEPS} steps", "hashes": {k: _run(mp, **kw)[0] for k, kw in RUNS.items()}}
    mp.undo()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
