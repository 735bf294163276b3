"""Round 5 GPU tests: what the window chain (csrc/window_pgs.h) owes the fused kernel besides the sweeps (odom velocity overwrite,
split-API statistics), the contact capacity of the small-free-body class beyond 64 contacts, and the solver check that bypasses the
oracle's own PGS."""
import os

import numpy as np
import pytest

import mujoco_sim_amd as ms
import orc
from helpers import oracle_s24

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _engine(m, nenv, window):
    lib = ms.capi.load()
    lib.mjh_set_window_solver(1 if window else 0)
    try:
        e = ms.Engine(m, nenv)
    finally:
        lib.mjh_set_window_solver(1)
    assert e.window_solver() == (1 if window else 0)
    return e


def test_odom_velocity_overwrite_in_the_window_chain(monkeypatch):
    """MjSim::set_odom_vels (mj_sim.cpp:1079-1153) runs behind mj_step2 whatever kernel integrates: a free box whose planar dofs are
    driven as odom dofs moves the same way through the window chain (assemble launch + mjh_window_kernel, the 16-row and the 32-row
    form) as through the fused kernel and the oracle (the window kernel used to skip the overwrite).  40 steps from
    reset: box 0 lands on the floor alone (the others are still falling), so the three trajectories are comparable to rounding."""
    m = ms.scene("s24")
    nenv = 8
    lin, ang, angq = [0, 1, -1], [-1, -1, 5], [-1, -1, -1]          # box 0: world x / y velocity and its body-z spin; no odom angle (free joints have none)
    twist = np.tile(np.array([[0.3, -0.2, 0, 0, 0, 0.7]]), (nenv, 1)) * np.linspace(0.5, 1.5, nenv)[:, None]
    outs = {}
    for name, window, w32 in (("window16", True, "0"), ("window32", True, "8"), ("fused", False, "0")):
        monkeypatch.setenv("MJH_WINDOW32", w32)
        e = _engine(m, nenv, window)
        tab = e.load_s24()
        e.set_odom(lin, ang, angq); e.set_odom_vel(twist)
        e.step(40)
        _, q, v, _ = e.get_state(); st = e.get_stats()
        e.step(110)
        _, q2, v2, _ = e.get_state()
        outs[name] = (q.copy(), v.copy(), st.copy(), q2.copy(), v2.copy())
        e.close()
    ref_q, ref_v = [], []
    for i in range(nenv):
        d = oracle_s24(m, tab, i)
        d.ifield("odom_lin")[:] = lin; d.ifield("odom_ang")[:] = ang; d.ifield("odom_angq")[:] = angq
        d.f("odom_vel")[:] = twist[i]
        d.step(40)
        ref_q.append(d.f("qpos").copy()); ref_v.append(d.f("qvel").copy())
    rq, rv = np.array(ref_q), np.array(ref_v)
    for name, (q, v, st, q2, v2) in outs.items():
        assert st[:, 0].min() >= 1, f"{name}: box 0 is on the floor, the sweeps ran"
        for vv in (v, v2):          # the overwritten dofs carry the command exactly, whatever the pile does later
            np.testing.assert_allclose(vv[:, [0, 1, 5]], twist[:, [0, 1, 5]], rtol=0, atol=1e-7, err_msg=name)
        np.testing.assert_allclose(q[:, :7], rq[:, :7], atol=1e-4, err_msg=name)            # the driven box against the oracle
        np.testing.assert_allclose(v[:, :6], rv[:, :6], atol=2e-3, err_msg=name)
        assert np.isfinite(q2).all()
    np.testing.assert_allclose(outs["window16"][0], outs["fused"][0], atol=1e-4)
    np.testing.assert_allclose(outs["window32"][0], outs["fused"][0], atol=1e-4)


def test_split_api_statistics_between_the_two_halves_are_this_steps():
    """mjh_step1 through the window chain hands every env over to mjh_step2; the contact / row counts mjh_get_stats returns between
    the two are those of THIS step's position stage, as after a plain mj_step1."""
    m = ms.scene("s24")
    nenv = 32
    e = _engine(m, nenv, True)
    e.load_s24()
    e.step(100)
    e.synchronize()
    _, q, v, w = e.get_state()
    f = _engine(m, nenv, False)
    f.load_s24()
    f.set_state(qpos=q, qvel=v, warmstart=w)
    # lift box 3 of every env out of contact: the counts of the next position stage differ from the last step's
    q2 = q.copy(); q2[:, 21 + 2] += 2.0
    e.set_state(qpos=q2); f.set_state(qpos=q2)
    before = e.get_stats()[:, :2].copy()
    e.step1(); f.step1()
    se, sf = e.get_stats(), f.get_stats()
    assert np.array_equal(se[:, :2], sf[:, :2]), "window hand-over and the fused step1 report the same counts"
    assert (se[:, 0] < before[:, 0]).any(), "and they are this step's (a box was lifted away)"
    e.step2(); f.step2()
    assert np.array_equal(e.get_stats()[:, :2], f.get_stats()[:, :2])
    e.close(); f.close()


# ---------------------------------------------------------------- S24D beyond 64 contacts (the "30-contact" scene without a capacity flag)
# bench.py's s24d seeds whose piles exceeded 64 contacts between steps 400 and 1400 of the r04 code (tools/r05_hist.py; 66 .. 68 contacts,
# 276 .. 300 rows) — the envs the 64-contact capacity of rounds 3 / 4 flagged and dropped contacts in
S24D_HEAVY_SEEDS = [1956, 2548, 2422, 375, 3623, 1290, 1556, 2278, 2967, 3149, 3445, 3669, 4044]
S24D_CAPACITY = 96


def _s24d_seeds(seeds, capacity=S24D_CAPACITY, window=True):
    """bench.py's S24D for the given env ids (per-env sizes / masses from the S24 seed of that id, released flat 2 x 2 with the id's yaws)"""
    pen = 0.175
    m = ms.scene("s24pen", pen, capacity)
    e = _engine(m, len(seeds), window)
    parts = [m.s24_randomize(int(s), 1) for s in seeds]
    tab = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
    q = tab["qpos"].reshape(len(seeds), 4, 7)
    for i, s in enumerate(seeds):
        rng = np.random.default_rng(0x524D0000 + int(s))
        for k in range(4):
            yaw = rng.uniform(-0.3, 0.3)
            q[i, k] = [(-1 if k & 1 else 1) * pen / 2, (-1 if k & 2 else 1) * pen / 2, 0.16 + 0.02 * k, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
    e.load_tables(tab)
    return m, e, tab


def test_s24d_capacity_above_64_contacts_takes_the_window_chain():
    """a small free-body model with a contact capacity of 65 .. 128 keeps the window chain (no contact-patch sweep: that one is tied to
    one contact per lane); its row capacity follows maxefc up to 24 windows"""
    m = ms.scene("s24pen", 0.175, S24D_CAPACITY)
    e = _engine(m, 8, True)
    assert e.window_solver() == 1 and e.patch_sweep() == 0 and e.solver_order() == 2
    e.close()
    m64 = ms.scene("s24pen", 0.175, 64)
    e = _engine(m64, 8, True)
    assert e.window_solver() == 1 and e.patch_sweep() == 1
    e.close()


def test_s24d_teacher_forced_including_the_envs_above_64_contacts():
    """the S24D envs that exceeded the 64-contact capacity, teacher-forced against the oracle.  64 envs — the 13 seeds
    above and the first 51 — settle 450 steps on the device (where the heavy seeds carry 60+ contacts), the oracles take the device's
    state over, then 100 steps teacher-forced at S24's tolerances with no capacity flag anywhere; the sample must contain env-steps
    with more than 64 contacts and with more than 256 rows (beyond the old row capacity as well)."""
    from test_gpu_teacher_forced import teacher_forced, summarize, S24_TOL_Q, S24_TOL_V
    seeds = S24D_HEAVY_SEEDS + list(range(51))
    m, e, tab = _s24d_seeds(seeds)
    e.step(450)
    t, q, v, w = e.get_state()
    st0 = e.get_stats()
    assert (st0[:, 3] & 3 == 0).all(), "no capacity flag while settling"
    ds = [oracle_s24(m, tab, i) for i in range(len(seeds))]
    for i, d in enumerate(ds):
        d.f("qpos")[:] = q[i]; d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = w[i]; d.f("time")[0] = t[i]
    r = teacher_forced(e, ds, 100)
    s = summarize("s24d-capacity96/default=mj_solPGS-row-order(window sweep), 13 seeds beyond 64 contacts + 51", r)
    a = r["agree"].astype(bool)
    heavy = r["ncon"] > 64
    print(f"S24D-HEAVY env-steps with > 64 contacts: {int(heavy.sum())} (agreeing {int((heavy & a).sum())}), max ncon {int(r['ncon'].max())}, max rows {int(r['nefc'].max())}, "
          f"env-steps with > 256 rows {int((r['nefc'] > 256).sum())}")
    for lo, hi in ((0, 128), (129, 192), (193, 256), (257, 400)):
        mk = a & (r["nefc"] >= lo) & (r["nefc"] <= hi)
        if mk.any():
            print(f"S24D-HEAVY rows {lo}-{hi}: {int(mk.sum())} env-steps, qpos max {r['eq'][mk].max():.2e}, qvel 99% {np.quantile(r['ev'][mk], 0.99):.2e} max {r['ev'][mk].max():.2e}, "
                  f"sweeps dev/oracle differ in {int((r['iter'][mk] != r['diter'][mk]).sum()) if 'diter' in r else -1}")
    worst = np.unravel_index(np.argmax(np.where(a, r["ev"], 0)), r["ev"].shape)
    print(f"S24D-HEAVY worst qvel env-step: step {worst[0]} env {worst[1]} (seed {seeds[worst[1]]}): ncon {int(r['ncon'][worst])} rows {int(r['nefc'][worst])} sweeps {int(r['iter'][worst])} ev {r['ev'][worst]:.2e} eq {r['eq'][worst]:.2e} ea {r['ea'][worst]:.2e}")
    assert heavy.sum() >= 20 and (heavy & a).sum() >= 10, "the sample must cover env-steps beyond the old contact capacity"
    assert r["nefc"].max() > 256
    assert s["agree_fraction"] >= 0.95, s
    # qpos at S24's tolerance; qvel: fp32 round-off at the 100-sweep cap grows with the row count (measured: max 1.3e-5 up to 128 rows,
    # 2.8e-5 up to 192, 8.6e-5 up to 256, 3.7e-5 beyond; 99 % 2.3e-5 in the worst class) — S24's 2e-5 for the 99 % quantile of the
    # whole sample, 5e-4 for its maximum (single outliers of 0.9e-4 .. 2.5e-4 among 6400 env-steps, depending on the window form the env
    # takes: the grouping of the arithmetic), the same bound for the env-steps beyond 64 contacts
    assert r["eq"][a].max() <= S24_TOL_Q and np.quantile(r["ev"][a], 0.99) <= S24_TOL_V and r["ev"][a].max() <= 5e-4, s
    assert r["eq"][heavy & a].max() <= S24_TOL_Q and r["ev"][heavy & a].max() <= 5e-4
    st = e.get_stats()
    assert (st[:, 3] & 3 == 0).all(), "no capacity flag"
    e.close()


def test_64_row_windows_for_the_envs_with_the_most_rows_equal_the_16_row_form_up_to_rounding(monkeypatch):
    """window_kernel.h wn_run64: S24D envs with more than 192 constraint rows (the ones a cohort's step waits for: 13 .. 19 windows of 16,
    every one at the 100-sweep cap) are swept in 64-row windows, one env per wavefront — same rows, same order, same stopping rule.
    Against the same engine with the section switched off (MJH_WINDOW64=0): the other envs are bitwise equal (their form did not
    change), the 64-row ones agree to fp32 rounding; and against the oracle one step from the device's state."""
    from test_gpu_teacher_forced import S24_TOL_Q
    nenv = 1024
    seeds = list(range(nenv))
    m, a, tab = _s24d_seeds(seeds)
    monkeypatch.setenv("MJH_WINDOW64", "0")
    _, b, _ = _s24d_seeds(seeds)
    monkeypatch.delenv("MJH_WINDOW64")
    a.step(420); a.synchronize()
    heavy_seen = 0; worst_q = worst_v = 0.0; same_it = []
    for k in range(30):
        t, q, v, w = a.get_state()
        b.set_state(qpos=q, qvel=v, time=t, warmstart=w)
        a.step(1); b.step(1)
        _, qa, va, _ = a.get_state(); _, qb, vb, _ = b.get_state()
        sa, sb = a.get_stats(), b.get_stats()
        assert np.array_equal(sa[:, :2], sb[:, :2]) and (sa[:, 3] & 3 == 0).all()
        heavy = (sa[:, 1] > 192) & (sa[:, 1] <= 320)
        assert np.array_equal(qa[~heavy], qb[~heavy]) and np.array_equal(va[~heavy], vb[~heavy]) and np.array_equal(sa[~heavy, 2], sb[~heavy, 2])
        if heavy.any():
            heavy_seen += int(heavy.sum())
            worst_q = max(worst_q, float((np.abs(qa[heavy] - qb[heavy]).max(1) / np.maximum(1, np.abs(qb[heavy]).max(1))).max()))
            worst_v = max(worst_v, float((np.abs(va[heavy] - vb[heavy]).max(1) / np.maximum(1, np.abs(vb[heavy]).max(1))).max()))
            same_it.append(float((sa[heavy, 2] == sb[heavy, 2]).mean()))
    tail_seen = int(((sa[:, 1] > 256) & (sa[:, 1] <= 320)).sum())
    print(f"WINDOW64: {heavy_seen} env-steps in 64-row windows of {30 * nenv}: qpos {worst_q:.2e} qvel {worst_v:.2e} against the 16-row form, same sweep count {np.mean(same_it):.3f}; envs beyond 256 rows (fifth window: tile in LDS) in the last step: {tail_seen}")
    assert heavy_seen >= 500 and worst_q <= S24_TOL_Q and worst_v <= 2e-4 and np.mean(same_it) >= 0.9
    # against the oracle: one step from the device's state, the envs in 64-row windows
    t, q, v, w = a.get_state()
    a.step(1); _, q1, v1, _ = a.get_state(); st = a.get_stats()
    tailed = np.nonzero((st[:, 1] > 256) & (st[:, 1] <= 320))[0][:8]
    heavy = np.concatenate([tailed, np.nonzero((st[:, 1] > 192) & (st[:, 1] <= 256))[0][:16 - len(tailed)]])
    assert len(heavy) >= 8
    eq = ev = 0.0
    for i in heavy:
        d = oracle_s24(m, tab, int(i))
        d.f("qpos")[:] = q[i]; d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = w[i]; d.f("qacc")[:] = w[i]; d.f("time")[0] = t[i]
        d.step(1)
        if d.i("ncon") != st[i, 0] or d.i("nefc") != st[i, 1]:
            continue
        eq = max(eq, float(np.abs(q1[i] - d.f("qpos")).max() / max(1, np.abs(d.f("qpos")).max())))
        ev = max(ev, float(np.abs(v1[i] - d.f("qvel")).max() / max(1, np.abs(d.f("qvel")).max())))
    print(f"WINDOW64 vs oracle, {len(heavy)} envs one step: qpos {eq:.2e} qvel {ev:.2e}")
    assert eq <= S24_TOL_Q and ev <= 2e-4
    a.close(); b.close()


# ---------------------------------------------------------------- the sweeps against an independent QP solve (no PGS of the oracle involved)
def _qp_check(m, mo, e, tab, nsettle, label, min_rows):
    """device state after nsettle steps -> per env: the oracle ASSEMBLES (J, AR = J M^-1 J^T + R, b = J qacc_smooth - aref) at that state, tests/qp_ref.py
    solves  min 1/2 f'AR f + b'f, f >= 0  exactly on the active set and certifies it (KKT residual <= 1e-10 max(1, |b|)), qacc* = qacc_smooth + M^-1 J^T f*; the device steps once with the sweep cap
    lifted (5000 sweeps, tolerance 0: the fixed point of its own fp32 sweeps) and returns its qacc (= the next warm start).  The
    problem is strictly convex (R > 0): the solution is unique, whatever the order or the form of the sweeps."""
    import qp_ref
    nenv = e.nenv
    e.step(nsettle); e.synchronize()
    t, q, v, w = e.get_state()
    e.step(1)
    _, _, _, qacc_dev = e.get_state(); st = e.get_stats()
    errs, rows, used = [], [], 0
    for i in range(nenv):
        d = oracle_s24(mo, tab, i)
        d.f("qpos")[:] = q[i]; d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = w[i]; d.f("time")[0] = t[i]
        d.call("step1"); d.call("fwd_acceleration"); d.call("fwd_constraint")
        n = d.i("nefc")
        if n != st[i, 1] or d.i("ncon") != st[i, 0] or n == 0:
            continue                                            # (another contact set: fp32 / fp64 narrow phase at a margin)
        AR, b, J, lo, hi = qp_ref.assemble(d, mo)
        f, res = qp_ref.solve(AR, b, lo, hi)
        if not qp_ref.certified(AR, b, res):
            continue                                            # (no certificate: not an instance)
        qacc_ref = qp_ref.qacc_of(d, J, f)
        errs.append(np.abs(qacc_dev[i] - qacc_ref).max() / max(1.0, np.abs(qacc_ref).max())); rows.append(n); used += 1
    errs = np.array(errs); rows = np.array(rows)
    print(f"QP-CHECK {label}: {used} of {nenv} instances ({int(rows.min())}..{int(rows.max())} rows, mean {rows.mean():.0f}; sweeps mean {st[:, 2].mean():.0f}): "
          f"qacc rel error median {np.median(errs):.2e} 99% {np.quantile(errs, 0.99):.2e} max {errs.max():.2e}")
    assert used >= 0.8 * nenv and rows.max() >= min_rows
    return errs


def test_window_sweeps_converge_to_the_qp_solution_of_an_independent_solver():
    """VERDICT r04 next #6c: >= 200 device instances (S24 through the 16- and 32-row forms, S24D through the tiers and the 64-row form) with
    the sweep cap lifted, against the certified optimum (tests/qp_ref.py) of the same quadratic program built from the oracle's constraint
    ASSEMBLY only (its own PGS takes no part).  fp32 fixed point against the fp64 optimum: qacc within 1e-3 relative at the median
    instance, 1e-2 at the worst."""
    def scene(name, cap, nenv):
        m = ms.scene("s24") if name == "s24" else ms.scene("s24pen", 0.175, cap)
        mo = ms.scene("s24") if name == "s24" else ms.scene("s24pen", 0.175, cap)
        m.c.opt.iterations = 5000; m.c.opt.tolerance = 0.0
        mo.c.opt.iterations = 1
        if name == "s24":
            e = _engine(m, nenv, True); tab = e.load_s24()
            return m, mo, e, tab
        lib = ms.capi.load()
        e = _engine(m, nenv, True)
        seeds = S24D_HEAVY_SEEDS[:8] + list(range(nenv - 8))
        parts = [m.s24_randomize(int(s), 1) for s in seeds]
        tab = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
        q = tab["qpos"].reshape(nenv, 4, 7)
        for i, s in enumerate(seeds):
            rng = np.random.default_rng(0x524D0000 + int(s))
            for k in range(4):
                yaw = rng.uniform(-0.3, 0.3)
                q[i, k] = [(-1 if k & 1 else 1) * 0.175 / 2, (-1 if k & 2 else 1) * 0.175 / 2, 0.16 + 0.02 * k, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        e.load_tables(tab)
        return m, mo, e, tab
    m, mo, e, tab = scene("s24", 0, 128)
    e1 = _qp_check(m, mo, e, tab, 300, "S24 (16- / 32-row windows)", 97)
    e.close()
    m, mo, e, tab = scene("s24d", S24D_CAPACITY, 96)
    e2 = _qp_check(m, mo, e, tab, 300, "S24D (tiers, 64-row windows)", 209)
    e.close()
    errs = np.concatenate([e1, e2])
    assert len(errs) >= 200
    assert np.median(errs) <= 1e-3 and errs.max() <= 1e-2          # measured: median 1.3e-4 (S24) / 3.9e-4 (S24D), max 1.8e-3 / 1.9e-3


@pytest.mark.parametrize("config", ["s24", "c2"])
def test_launch_chain_as_a_captured_graph_equals_the_separate_launches(config):
    """B2 (one launch per step): where a cohort-step is a chain of launches — the window chain (assemble -> window kernel) and
    the many-body layout (assemble -> solve -> integrate) — mjh_step queues it as ONE captured graph per cohort-step
    (mjh_launches_per_step == 1; default for the many-body chain, opt-in — mode 2 — for the window chain, where it measures 2 % slower).  Same kernels, same arguments: bitwise the state of the separate launches, over order renewals, a
    state change between calls (set_state: nothing the graph holds by value) and a change of what it does hold (the cohort count)."""
    lib = ms.capi.load()
    outs = []
    for graph in (2, 0):
        lib.mjh_set_chain_graph(graph)
        try:
            if config == "s24":
                m = ms.scene("s24"); nenv = 1536
                e = ms.Engine(m, nenv); e.load_s24()
            else:
                m = ms.scene("boxpile", 64); m.c.maxcon = 600; m.c.maxefc = 2400          # bench.py's C2
                nenv = 1536
                e = ms.Engine(m, nenv)
                e.load_tables(ms.boxes_randomize(m, 0, nenv, jitter=0.01))
            e.set_cohorts(3)
            assert e.launches_per_step == (1 if graph else (2 if config == "s24" else 3))
            e.step(40)
            t, q, v, w = e.get_state()
            e.set_state(qvel=v * 0.5)                # (the graphs stay valid: the state lives behind pointers)
            e.step(37, True)
            e.set_cohorts(2)                         # (env ranges of the cohorts change: captured again)
            e.step(10)
            outs.append((e.get_state(), e.get_stats()[:, :3].copy()))
            e.close()
        finally:
            lib.mjh_set_chain_graph(1)
    (sa, sta), (sb, stb) = outs
    for x, y in zip(sa, sb):
        assert np.array_equal(x, y)
    assert np.array_equal(sta, stb) and sta[:, 0].mean() > 4


def test_s24d_results_do_not_depend_on_cohorts_launch_order_or_batch_size():
    """every env's arithmetic stays inside its own lanes in all three window forms (16-row: a 16-lane row of a four-env wavefront; 32-row: half
    a wavefront; 64-row: a wavefront of its own, tiles of the last windows in that workgroup's LDS), and the form is a function of the env's
    own row count: S24D (all three forms, tiers, up to ~280 rows) gives the same bits on 1 / 3 / 2 cohorts (the launch order — window count
    first, sweeps second — is sorted per cohort: which envs share a wavefront changes with them), another batch size and other call lengths"""
    outs = []
    for nenv, nc, chunk in ((1280, 1, 430), (1280, 3, 7), (1283, 2, 43)):
        m, e, tab = _s24d_seeds(list(range(nenv)))
        e.set_cohorts(nc)
        for _ in range(0, 430, chunk):
            e.step(min(chunk, 430 - _))
        t, q, v, w = e.get_state(); st = e.get_stats()
        outs.append((q[:1280], v[:1280], w[:1280], st[:1280, :3]))
        assert (st[:, 3] & 7 == 0).all()
        e.close()
    rows = outs[0][3][:, 1]
    assert (rows > 208).sum() >= 10 and ((rows > 96) & (rows <= 128)).sum() >= 50 and (rows <= 96).sum() >= 20, "all three forms present"
    for k in (1, 2):
        for x, y in zip(outs[0], outs[k]):
            assert np.array_equal(x, y)


def test_s24_64_row_windows_for_the_envs_beyond_96_rows_equal_the_16_row_form_up_to_rounding(monkeypatch):
    """S24's default since round 5: envs with more than 96 rows (9 % — the ones a cohort's step waits for) are swept in 64-row windows, one env
    per wavefront, both windows register-resident, the chains' wait states filled.  Against the same engine with both wide sections off
    (every env in the 16-row form): the others bitwise equal, the 64-row envs equal to fp32 rounding with the same sweep counts; and
    against the oracle one step from the device's state."""
    from test_gpu_teacher_forced import S24_TOL_Q, S24_TOL_V
    m = ms.scene("s24")
    nenv = 2048
    a = ms.Engine(m, nenv); tab = a.load_s24()
    monkeypatch.setenv("MJH_WINDOW64", "0"); monkeypatch.setenv("MJH_WINDOW32", "0")
    b = ms.Engine(m, nenv); b.load_s24()
    monkeypatch.delenv("MJH_WINDOW64"); monkeypatch.delenv("MJH_WINDOW32")
    a.step(300); a.synchronize()
    heavy_seen = 0; worst_q = worst_v = 0.0; same_it = []
    for k in range(40):
        t, q, v, w = a.get_state()
        b.set_state(qpos=q, qvel=v, time=t, warmstart=w)
        a.step(1); b.step(1)
        _, qa, va, _ = a.get_state(); _, qb, vb, _ = b.get_state()
        sa, sb = a.get_stats(), b.get_stats()
        assert np.array_equal(sa[:, :2], sb[:, :2])
        heavy = sa[:, 1] > 96
        assert np.array_equal(qa[~heavy], qb[~heavy]) and np.array_equal(va[~heavy], vb[~heavy]) and np.array_equal(sa[~heavy, 2], sb[~heavy, 2])
        if heavy.any():
            heavy_seen += int(heavy.sum())
            worst_q = max(worst_q, float((np.abs(qa[heavy] - qb[heavy]).max(1) / np.maximum(1, np.abs(qb[heavy]).max(1))).max()))
            worst_v = max(worst_v, float((np.abs(va[heavy] - vb[heavy]).max(1) / np.maximum(1, np.abs(vb[heavy]).max(1))).max()))
            same_it.append(float((sa[heavy, 2] == sb[heavy, 2]).mean()))
    print(f"S24-WINDOW64: {heavy_seen} env-steps in 64-row windows of {40 * nenv}: qpos {worst_q:.2e} qvel {worst_v:.2e} against the 16-row form, same sweep count {np.mean(same_it):.3f}")
    assert heavy_seen >= 400 and worst_q <= S24_TOL_Q and worst_v <= S24_TOL_V and np.mean(same_it) >= 0.9
    t, q, v, w = a.get_state()
    a.step(1); _, q1, v1, _ = a.get_state(); st = a.get_stats()
    heavy = np.nonzero(st[:, 1] > 96)[0][:24]
    assert len(heavy) >= 8
    checked = 0
    for i in heavy:
        d = oracle_s24(m, tab, int(i))
        d.f("qpos")[:] = q[i]; d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = w[i]; d.f("qacc")[:] = w[i]; d.f("time")[0] = t[i]
        d.step(1)
        if d.i("ncon") != st[i, 0] or d.i("nefc") != st[i, 1]:
            continue
        checked += 1
        assert np.abs(q1[i] - d.f("qpos")).max() / max(1, np.abs(d.f("qpos")).max()) <= S24_TOL_Q
        assert np.abs(v1[i] - d.f("qvel")).max() / max(1, np.abs(d.f("qvel")).max()) <= S24_TOL_V
    assert checked >= 6
    a.close(); b.close()


def test_s24d_assemble_only_launch_with_its_scratch_in_the_dead_contact_records():
    """The assemble-only instance of window-only models (65 .. 128 contacts) allocates no LDS for the block schedule, the condim-4 extension and
    the per-base scratch vectors bv / phi: no schedule is built, and bv / phi (velocity stage: J qvel -> aref; mj_inverse: J qacc, base forces)
    live in the contact records, dead once the rows are made (engine.hip: lds_bytes_pre; step_kernel.h: WPRE == 2).  Against the fused kernel
    (own slots for all of them, MJH_WINDOW off) on the same states: mj_inverse's output after one step and the split API's hand-over."""
    lib = ms.capi.load()
    m = ms.scene("s24pen", 0.175, S24D_CAPACITY)
    full, pre = lib.mjh_query_lds_bytes(m.ptr), lib.mjh_query_lds_bytes_assemble(m.ptr)
    assert 0 < pre <= 17 * 1024 < full, (pre, full)           # (25.3 KB before: six environments per CU; now nine)
    seeds = list(range(48))
    _, a, _ = _s24d_seeds(seeds, window=True)
    _, b, _ = _s24d_seeds(seeds, window=False)
    a.step(300); t, q, v, w = a.get_state()
    b.set_state(qpos=q, qvel=v, time=t, warmstart=w)
    st = a.get_stats()
    assert st[:, 0].max() > 24 and (st[:, 3] & 7 == 0).all()
    a.step(1, True); b.step(1, True)
    fa, fb = a.get_field("qfrc_inverse"), b.get_field("qfrc_inverse")
    scale = np.abs(fb).max()
    assert scale > 1.0 and np.abs(fa - fb).max() <= 2e-3 * scale, (np.abs(fa - fb).max(), scale)
    # split API: mjh_step1 + mjh_inverse is the assemble-only launch with the hand-over; mjh_step2 the window kernel
    t, q, v, w = a.get_state()
    b.set_state(qpos=q, qvel=v, time=t, warmstart=w)
    a.step1(); a.inverse(); b.step1(); b.inverse()
    fa, fb = a.get_field("qfrc_inverse"), b.get_field("qfrc_inverse")
    assert np.abs(fa - fb).max() <= 2e-3 * max(np.abs(fb).max(), 1.0)
    a.step2(); b.step2()
    _, q1, v1, _ = a.get_state(); _, q2, v2, _ = b.get_state()
    assert np.abs(q1 - q2).max() <= 5e-6 and np.abs(v1 - v2).max() <= 2e-3
    a.close(); b.close()
