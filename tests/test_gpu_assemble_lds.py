"""GPU tests of the slim assemble-only LDS extent of patch models (engine.hip: DWpre; step_kernel.h: WPRE instance 1 keeps bv / phi in the contact
records and its base rows where the fused layout has bv, phi and the pair schedule): the new layout against the former one
(MJH_WPRE_SLIM3=0), bit for bit, and against the fp64 oracle.  The knob is read when the first engine of a process is created, so each
engine runs in a fresh child process that leaves its arrays in a file."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mujoco_sim_amd as ms
from conftest import ROOT
from helpers import oracle_s24

pytestmark = pytest.mark.gpu

NENV, COHORTS = 256, 3          # the smallest count at which the cohort path (nenv >= 64 * cohorts) and the launch order are live
TOL_Q, TOL_V = 1e-6, 2e-5       # tests/test_gpu_window_lean.py's bounds against the oracle (relative to max(1, |x|))

_SCRIPT = r"""
import sys
sys.path.insert(0, {root!r})
import numpy as np
import mujoco_sim_amd as ms
case, out = sys.argv[1], sys.argv[2]
m = ms.scene("s24")
if case == "capacity":
    m.c.maxcon = 16; m.c.maxefc = 96
e = ms.Engine(m, {nenv})
assert e.window_solver() == 1
e.load_s24(); e.set_cohorts({cohorts})
import ctypes as C
buf = C.create_string_buffer(8192)
assert ms.capi.load().mjh_debug_lds_layout(m.ptr, buf, 8192) > 0
res = dict(assemble_bytes=np.array([int(buf.value.decode().split("lds_bytes_wpre")[1].split()[0])]))          # what the assemble-only launch allocates
def snap(tag):
    e.synchronize()
    t, q, v, w = e.get_state(); st = e.get_stats()
    res.update({{tag + "_time": t.copy(), tag + "_qpos": q.copy(), tag + "_qvel": v.copy(), tag + "_ws": w.copy(), tag + "_stats": st.copy()}})
if case == "landing":
    e.step(1); snap("first")
    e.step(149); snap("end")
    e.step(1); snap("next")
else:
    e.step(60); snap("end")
e.close()
np.savez(out, **res)
"""


def _run(case, slim3, tmp_path):
    env = dict(os.environ)
    env.pop("MJH_WPRE_SLIM3", None)
    if slim3 is not None:
        env["MJH_WPRE_SLIM3"] = str(slim3)
    out = str(tmp_path / f"{case}_{slim3}.npz")
    r = subprocess.run([sys.executable, "-c", _SCRIPT.format(root=ROOT, nenv=NENV, cohorts=COHORTS), case, out], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return dict(np.load(out))


def _same(a, b, tag):
    for k in ("time", "qpos", "qvel", "ws", "stats"):
        x, y = a[f"{tag}_{k}"], b[f"{tag}_{k}"]
        assert np.array_equal(x, y), f"{tag}_{k}: {int((x != y).reshape(len(x), -1).any(axis=1).sum())} envs differ"


@pytest.fixture(scope="module")
def landing(tmp_path_factory):
    d = tmp_path_factory.mktemp("assemble_lds")
    return _run("landing", None, d), _run("landing", 0, d)


def test_landing_boxes_new_layout_equals_the_former_bitwise(landing):
    """S24, 256 envs on three cohorts, 150 steps from the drop: every env goes from no contact to its peak while the boxes land."""
    new, old = landing
    assert int(new["assemble_bytes"][0]) <= 13 * 1280 < int(old["assemble_bytes"][0]), "the two runs are the two layouts"
    first, ncon = new["first_stats"][:, 0], new["end_stats"][:, 0]
    print(f"ASSEMBLE-LDS landing: contacts in the first step min {first.min()} mean {first.mean():.1f} max {first.max()}, "
          f"after 150 steps min {ncon.min()} mean {ncon.mean():.1f} max {ncon.max()}, rows max {new['end_stats'][:, 1].max()}")
    assert (first == 0).any() and (ncon > 0).all() and ncon.mean() > first.mean(),"the run goes from released boxes (some envs without a contact) to landed ones"
    for tag in ("first", "end", "next"):
        _same(new, old, tag)


def test_full_contact_pools_new_layout_equals_the_former_bitwise(tmp_path):
    """The same scene with 16 contacts / 96 rows of capacity, 60 steps: envs overflow, and an overlay that aliased a live array would show first
    with the pools full.  Bitwise equal, overflow flags included; at least one env carries the flag."""
    new, old = _run("capacity", None, tmp_path), _run("capacity", 0, tmp_path)
    assert int(new["assemble_bytes"][0]) < int(old["assemble_bytes"][0])
    flags = new["end_stats"][:, 3] & 3          # 1: contacts beyond maxcon dropped, 2: rows beyond the capacity dropped
    print(f"ASSEMBLE-LDS capacity: envs with an overflow flag {int((flags != 0).sum())} of {NENV}, contacts max {new['end_stats'][:, 0].max()}")
    assert (flags != 0).any(), "no env overflowed: the case is empty"
    _same(new, old, "end")
    assert np.array_equal(new["end_stats"][:, 3] & 0xff, old["end_stats"][:, 3] & 0xff)


def test_one_step_of_the_new_layout_against_the_oracle(landing):
    """32 envs of the landing case, one step from the state the 150 steps left (contacts present), against the fp64 oracle."""
    new, _ = landing
    m = ms.scene("s24")
    tab = m.s24_randomize(0, NENV)
    st = new["next_stats"]
    worst_q = worst_v = 0.0
    checked = 0
    for i in range(32):
        d = oracle_s24(m, tab, i)
        d.f("qpos")[:] = new["end_qpos"][i]; d.f("qvel")[:] = new["end_qvel"][i]; d.f("qacc_warmstart")[:] = new["end_ws"][i]; d.f("qacc")[:] = new["end_ws"][i]
        d.f("time")[0] = new["end_time"][i]
        d.step(1)
        if d.i("ncon") != st[i, 0] or d.i("nefc") != st[i, 1]:
            continue          # (a contact at the margin seen by one side only: not the same problem — as in tests/test_gpu_window_lean.py)
        eq = float(np.abs(new["next_qpos"][i] - d.f("qpos")).max() / max(1, np.abs(d.f("qpos")).max()))
        ev = float(np.abs(new["next_qvel"][i] - d.f("qvel")).max() / max(1, np.abs(d.f("qvel")).max()))
        worst_q = max(worst_q, eq); worst_v = max(worst_v, ev); checked += 1
    print(f"ASSEMBLE-LDS vs oracle: checked {checked} of 32, worst qpos {worst_q:.2e} qvel {worst_v:.2e}")
    assert checked >= 24, "a contact at the margin is rare: at least three quarters of the envs pose the same problem to both sides"
    assert worst_q <= TOL_Q and worst_v <= TOL_V
