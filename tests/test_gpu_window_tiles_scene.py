"""GPU tests of the window kernel with its tile rows built on the matrix cores (csrc/window_tiles.h), in the scenes that reach every
tile build: the state is, bit for bit, what the library of the commit before computed, and one step matches the fp64 oracle.

(a) The scene of tests/test_gpu_window_straight.py / test_gpu_window_slots.py — S24's model class in a pen, 256 envs in three cohorts, 150
    steps: wavefronts of every window count 1 .. 6 (single tiles, pairs with their cross tile) and envs of 97 .. 128 rows (the 64-row
    form's register windows); hashes: tests/golden/window_slots_hashes.json, recorded from a library with the broadcast multiply-add tiles.
(b) The pen scene of tests/test_gpu_window_lean.py — every env released flat 2 x 2 at a capacity of 256 rows, 60 steps: envs of 129 .. 192
    rows (the 64-row form's LDS-tile window in the lean instance, its third register window in the fat one) and beyond 192 (the 16-row
    form's tier windows and their cross tiles), forced lean and forced fat; hashes: tests/golden/window_tiles_hashes.json, recorded from
    the parent commit's library (`python tests/test_gpu_window_tiles_scene.py OUT.json COMMIT` with MJHIP_LIB naming that library).
(c) In both scenes 32 envs, one step from the state after 60 steps against the oracle: qpos 1e-6, qvel 2e-5 relative to max(1, |x|), the
    bounds of tests/test_gpu_window_lean.py."""
import json
import os
import sys

import numpy as np
import pytest

from test_gpu_window_slots import GOLDEN as SLOTS_GOLDEN, NW, _run as _run_straight, _sha, _wave_windows
from test_gpu_window_slots import _engine as _engine_straight
from test_gpu_window_lean import _engine as _engine_pen

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_tiles_hashes.json")
PEN_NENV, PEN_STEPS = 512, 60
TOL_Q, TOL_V = 1e-6, 2e-5


def _run_pen(monkeypatch, lean):
    """-> ({array name: sha256} after PEN_STEPS steps, env-steps with 129 .. 192 rows, env-steps beyond 192 rows)"""
    m, e, tab = _engine_pen(PEN_NENV, lean, monkeypatch)
    n129 = n193 = 0
    for _ in range(PEN_STEPS):
        e.step(1)
        r = e.get_stats()[:, 1]
        n129 += int(((r > 128) & (r <= 192)).sum()); n193 += int((r > 192).sum())
    e.synchronize()
    t, q, v, w = e.get_state(); st = e.get_stats()
    h = {"qpos": _sha(q), "qvel": _sha(v), "qacc_warmstart": _sha(w), "stats": _sha(st[:, :3].astype(np.int32)), "flags": _sha((st[:, 3] & 0xff).astype(np.int32))}
    e.close()
    return h, n129, n193


def _one_step_against_the_oracle(m, e, tab, nenv, name):
    from helpers import oracle_s24
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
    rows = st[:, 1]
    print(f"WINDOW-TILES {name} vs oracle: {checked} of {nenv} envs, rows {int(rows.min())} .. {int(rows.max())}, worst qpos {worst_q:.2e} qvel {worst_v:.2e}")
    e.close()
    return checked, worst_q, worst_v, rows


def test_straight_scene_is_bitwise_the_broadcast_tiles(monkeypatch):
    with open(SLOTS_GOLDEN) as f:
        golden = json.load(f)
    h, rows = _run_straight(monkeypatch)
    form64 = (rows > 96) & (rows <= 192)
    counts = np.bincount(_wave_windows(rows, form64).ravel(), minlength=NW + 1)
    n64 = int(((rows > 96) & (rows <= 128)).sum())
    print(f"WINDOW-TILES: wavefront-steps by largest window count 0 .. : {counts.tolist()}; env-steps with 97 .. 128 rows: {n64}; hashes {h}")
    assert all(counts[k] > 0 for k in range(1, NW + 1)), "wavefronts of every window count 1 .. 6 must occur"
    assert n64 > 0, "some envs must reach 97 .. 128 rows and take the 64-row form"
    assert h == golden["hashes"]["default"]


@pytest.mark.parametrize("name,lean", [("pen_lean", 1), ("pen_fat", 0)])
def test_pen_scene_is_bitwise_the_parents(monkeypatch, name, lean):
    with open(GOLDEN) as f:
        golden = json.load(f)
    h, n129, n193 = _run_pen(monkeypatch, lean)
    print(f"WINDOW-TILES {name}: env-steps with 129 .. 192 rows: {n129}, beyond 192: {n193} of {PEN_NENV * PEN_STEPS}; hashes {h}")
    assert n129 > 0 and n193 > 0, "the run must contain envs of 129 .. 192 rows and beyond 192 rows"
    assert h == golden["hashes"][name]


def test_straight_scene_one_step_against_the_oracle(monkeypatch):
    nenv = 32
    m, e, tab = _engine_straight(monkeypatch, nenv=nenv, nflat=8)
    checked, worst_q, worst_v, rows = _one_step_against_the_oracle(m, e, tab, nenv, "straight scene")
    assert checked >= nenv // 2
    assert worst_q <= TOL_Q and worst_v <= TOL_V


def test_pen_scene_one_step_against_the_oracle(monkeypatch):
    nenv = 32
    m, e, tab = _engine_pen(nenv, 1, monkeypatch)
    checked, worst_q, worst_v, rows = _one_step_against_the_oracle(m, e, tab, nenv, "pen scene")
    assert rows.max() > 128, "envs beyond 128 rows"
    assert checked >= nenv // 2
    assert worst_q <= TOL_Q and worst_v <= TOL_V


if __name__ == "__main__":      # record the pen scene's hashes with the library in use (MJHIP_LIB selects a build): python tests/test_gpu_window_tiles_scene.py OUT.json [commit id]
    mp = pytest.MonkeyPatch()
    runs = {name: _run_pen(mp, lean) for name, lean in (("pen_lean", 1), ("pen_fat", 0))}
    out = {"parent_commit": sys.argv[2] if len(sys.argv) > 2 else "",
           "produced_by": "python tests/test_gpu_window_tiles_scene.py OUT.json COMMIT, on one MI355X, with the library built from that commit",
           "scene": f"s24pen 0.175 64 released flat 2 x 2, MJH_WINDOW_MAXW=16, {PEN_NENV} envs, {PEN_STEPS} steps, MJH_WINDOW_LEAN=1 / 0",
           "env_steps_129_192_rows": {k: r[1] for k, r in runs.items()}, "env_steps_beyond_192_rows": {k: r[2] for k, r in runs.items()},
           "hashes": {k: r[0] for k, r in runs.items()}}
    mp.undo()
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out, indent=1))
