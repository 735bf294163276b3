"""GPU test of the collision stage of the window chain's assemble-only instances (csrc/step_kernel.h collide_round: the contact emit with
lanes = contacts): count, order and every record of every env's contact list are, bit for bit, what the library of the commit before
computed with the per-pair emit loop.

mjh_get_contacts takes its snapshot of a window-chain model through the assemble-only instance (the collision code the model's steps run),
so the lists below come from the code under test.  Scenes:
(a) S24 from the drop, 64 envs in three cohorts, the lists after 1, 40 and 150 steps (the release poses already touch in places, the
    boxes land and tumble, the piles have settled: edge-edge points at every one of them, full 8-point box-box manifolds at the last);
(b) the pen scene of tests/test_gpu_window_lean.py (every env released flat 2 x 2, contact capacity 64), 64 envs, after 60 steps.
tests/golden/collide_lanes_contacts.json holds, per scene and step, the contact count of every env and the SHA-256 of all records (dist,
pos, frame, geoms in list order), recorded from the parent commit's library — its snapshot ran the fused instance's per-pair loop —
with `python tests/test_gpu_collide_lanes.py OUT.json COMMIT` (MJHIP_LIB naming that library), and how many box-box pairs of the free
boxes carry 8 points and how many an edge-edge point: both must occur, or the scene would not exercise the emit's longest lists."""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import mujoco_sim_amd as ms

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collide_lanes_contacts.json")
NENV, NCOHORT = 64, 3
S24_STEPS, PEN_STEP = (1, 40, 150), 60
FIRST_FREE_BOX = 5        # geoms 0 .. 4: the pen (floor and walls); 5 .. 8: the four free boxes, one per body


def _quat_mat(q):
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1-2*(y*y+z*z), 2*(x*y-w*z), 2*(x*z+w*y)], [2*(x*y+w*z), 1-2*(x*x+z*z), 2*(y*z-w*x)], [2*(x*z-w*y), 2*(y*z+w*x), 1-2*(x*x+y*y)]])


def _snapshot(e):
    """-> {"counts": [per env], "sha256": of all records, "manifold8": pairs of free boxes with 8 points, "edge_edge": such pairs with one
    point whose normal is an axis of neither box}"""
    nenv = e.nenv
    _, q, _, _ = e.get_state()
    h = hashlib.sha256()
    counts, n8, nedge = [], 0, 0
    for i in range(nenv):
        c = e.get_contacts(i)
        counts.append(int(len(c["dist"])))
        for k in ("dist", "pos", "frame", "geom"):
            h.update(np.ascontiguousarray(c[k]).tobytes())
        by = {}
        for k in range(len(c["dist"])):
            g1, g2 = (int(x) for x in c["geom"][k])
            if g1 >= FIRST_FREE_BOX and g2 >= FIRST_FREE_BOX:
                by.setdefault((g1, g2), []).append(k)
        for (g1, g2), ks in by.items():
            assert ks == list(range(ks[0], ks[0] + len(ks))), "a pair's contacts are consecutive"
            if len(ks) == 8:
                n8 += 1
            if len(ks) == 1:
                n = c["frame"][ks[0], :3]
                axes = np.concatenate([_quat_mat(q[i].reshape(-1, 7)[g - FIRST_FREE_BOX, 3:]).T for g in (g1, g2)])
                if np.abs(axes @ n).max() < 0.99:
                    nedge += 1
    return {"counts": counts, "sha256": h.hexdigest(), "manifold8": n8, "edge_edge": nedge}


def _run_s24():
    m = ms.scene("s24")
    e = ms.Engine(m, NENV)
    e.load_s24()
    e.set_cohorts(NCOHORT)
    assert e.window_solver() == 1
    out, done = {}, 0
    for s in S24_STEPS:
        e.step(s - done); e.synchronize(); done = s
        out[f"s24_step{s}"] = _snapshot(e)
    e.close()
    return out


def _run_pen(monkeypatch):
    from test_gpu_window_lean import _engine as _engine_pen
    m, e, tab = _engine_pen(NENV, 1, monkeypatch)
    e.step(PEN_STEP); e.synchronize()
    out = {f"pen_step{PEN_STEP}": _snapshot(e)}
    e.close()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _compare(got, golden):
    for key, snap in got.items():
        want = golden["snapshots"][key]
        print(f"COLLIDE-LANES {key}: contacts {sum(snap['counts'])} (max {max(snap['counts'])} per env), 8-point box-box manifolds {snap['manifold8']}, "
              f"edge-edge points {snap['edge_edge']}, sha256 {snap['sha256'][:16]} (golden {want['sha256'][:16]})")
        assert snap["counts"] == want["counts"], f"{key}: contact counts differ"
        assert snap["sha256"] == want["sha256"], f"{key}: a contact record differs"


def test_s24_contact_lists_are_bitwise_the_parents(golden):
    snaps = golden["snapshots"]
    assert sum(snaps[f"s24_step{s}"]["manifold8"] for s in S24_STEPS) > 0, "the golden run must contain an 8-point box-box manifold"
    assert sum(snaps[f"s24_step{s}"]["edge_edge"] for s in S24_STEPS) > 0, "the golden run must contain an edge-edge contact"
    _compare(_run_s24(), golden)


def test_pen_scene_contact_lists_are_bitwise_the_parents(golden, monkeypatch):
    _compare(_run_pen(monkeypatch), golden)


if __name__ == "__main__":      # record the golden with the library in use (MJHIP_LIB selects a build): python tests/test_gpu_collide_lanes.py OUT.json [commit id]
    mp = pytest.MonkeyPatch()
    snaps = _run_s24(); snaps.update(_run_pen(mp))
    mp.undo()
    out = {"parent_commit": sys.argv[2] if len(sys.argv) > 2 else "",
           "produced_by": "python tests/test_gpu_collide_lanes.py OUT.json COMMIT, on one MI355X, with the library built from that commit",
           "scenes": f"s24 from the drop, {NENV} envs, {NCOHORT} cohorts, steps {list(S24_STEPS)}; s24pen 0.175 64 released flat 2 x 2, MJH_WINDOW_MAXW=16, {NENV} envs, step {PEN_STEP}",
           "snapshots": snaps}
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({k: {kk: vv for kk, vv in v.items() if kk != "counts"} for k, v in snaps.items()}, indent=1))
