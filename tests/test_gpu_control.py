"""The loop on the device: mjh_set_cmd_device, mjh_set_pd_target_device, mjh_set_xfrc_applied_device, mjh_get_joint_state_device,
mjh_reset_device and mjh_reset with an id list, against the host entry points.

Twin engines of one model: A is driven through the host entry points, B through the device ones with the same fp32 values (A gets them as
float64 copies, which the host path rounds back to the same floats).  The device path copies bits, so every comparison is array_equal on
get_state (time, qpos, qvel, warm start), get_stats and get_field("qacc") of ALL envs: the envs outside a range or a mask must not move.
Shapes are the smallest at which the code can still go wrong: sub-ranges, a mask with holes, nq != nv, nv beyond one wavefront's 64 lanes
(boxpile(11), nv 66), the window chain's split API (S24), two cohorts with forked streams."""
import ctypes as C

import numpy as np
import pytest
import torch

import contact_scenes as cs
import frame_scenes as fs
import mujoco_sim_amd as ms

pytestmark = pytest.mark.gpu
NENV = 6
MASK = [0, 1, 0, 0, 1, 1]
IDS = [1, 4, 5]
MJH_ERR_STATE = -4


def _dev(a, dtype=torch.float32):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype).cuda()
    torch.cuda.synchronize()
    return t


def _f32(rng, shape, lo=-1.0, hi=1.0):
    """fp32 values and their float64 copies (what the host twin is given)"""
    a = rng.uniform(lo, hi, shape).astype(np.float32)
    return a, a.astype(np.float64)


def _snap(e):
    e.synchronize()
    t, q, v, w = e.get_state()
    return dict(time=t, qpos=q, qvel=v, warmstart=w, stats=e.get_stats(), qacc=e.get_field("qacc"))


def _same(A, B, what):
    a, b = _snap(A), _snap(B)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=f"{what}: {k}")
    assert np.isfinite(b["qpos"]).all() and np.isfinite(b["qvel"]).all(), what


def _twins(name, nenv=NENV, **kw):
    """two engines of one model in the same state, every env different from the others"""
    rng = np.random.default_rng(17)
    if name == "s24":
        m = ms.scene("s24")
    elif name == "arm7":
        m = ms.scene("arm7", 1)
    else:
        m = ms.scene("boxpile", 11)
        assert m.nv == 66
    q0 = np.tile(m.array("qpos0"), (nenv, 1))
    if name == "arm7":
        q0 = q0 + rng.uniform(-0.05, 0.05, q0.shape)
        v0 = rng.uniform(-0.5, 0.5, (nenv, m.nv))
    elif name == "pile":
        q0.reshape(nenv, -1, 7)[:, :, :2] += rng.uniform(-0.004, 0.004, (nenv, m.nq // 7, 2))
    out = []
    for _ in range(2):
        e = ms.Engine(m, nenv, **kw)
        if name == "s24":
            e.load_s24()
        else:
            e.set_initial_qpos(q0); e.reset()
            if name == "arm7":
                e.set_state(qvel=v0)
        out.append(e)
    return m, out[0], out[1]


def _close(*es):
    for e in es:
        e.close()


# ------------------------------------------------------------------ 1. commands
@pytest.mark.parametrize("which", ["ddq", "dq", "both"])
def test_commands_on_a_sub_range(which):
    m, A, B = _twins("arm7")
    rng = np.random.default_rng(3)
    a32, a64 = _f32(rng, (3, m.nv), -2, 2); b32, b64 = _f32(rng, (3, m.nv), -0.3, 0.3)
    da, db = _dev(a32), _dev(b32)
    use_a, use_b = which != "dq", which != "ddq"
    for k in range(2):
        A.set_cmd(a64 if use_a else None, b64 if use_b else None, env0=1)
        B.set_cmd_device(da if use_a else None, db if use_b else None, env0=1)
        A.step(); B.step()
        _same(A, B, f"{which}, step {k}")
    B.set_cmd_device(None, None, env0=1, n=3)      # no-op
    A.step(); B.step()
    _same(A, B, "after the no-op")
    _close(A, B)


def test_commands_between_step1_and_step2_keep_the_hand_over():
    m, A, B = _twins("s24")
    rng = np.random.default_rng(4)
    A.step(3); B.step(3)
    for k in range(3):
        a32, a64 = _f32(rng, (3, m.nv), -3, 3); b32, b64 = _f32(rng, (3, m.nv), -0.2, 0.2)
        da, db = _dev(a32), _dev(b32)
        A.step1(); B.step1()
        A.set_cmd(a64, b64, env0=1); B.set_cmd_device(da, db, env0=1)
        A.step2(); B.step2()
        _same(A, B, f"split step {k}")
    _close(A, B)


# ------------------------------------------------------------------ 2. PD targets and xfrc_applied
def test_pd_targets_with_the_in_kernel_step_loop(lib):
    m, A, B = _twins("arm7")
    rng = np.random.default_rng(5)
    t32, t64 = _f32(rng, (4, m.nv), -0.3, 0.3)
    t32 = (t32 + m.array("qpos0").astype(np.float32)).astype(np.float32); t64 = t32.astype(np.float64)
    dt = _dev(t32)
    assert lib.mjh_set_pd_target_device(B.h, 2, 4, C.c_void_p(dt.data_ptr())) == MJH_ERR_STATE      # controller off
    for e in (A, B):
        e.set_pd_controller(200.0, 50.0)
    A.set_pd_target(t64, env0=2); B.set_pd_target_device(dt, env0=2)
    A.step(4); B.step(4)
    _same(A, B, "PD targets")
    _close(A, B)


def test_xfrc_applied_with_the_first_use_allocation():
    m, A, B = _twins("s24")
    rng = np.random.default_rng(6)
    x32, x64 = _f32(rng, (4, m.nbody, 6), -20, 20)
    dx = _dev(x32)
    A.step(2); B.step(2)
    A.set_xfrc_applied(x64, env0=1); B.set_xfrc_applied_device(dx, env0=1)      # allocates in both twins
    np.testing.assert_array_equal(A.get_xfrc_applied(), B.get_xfrc_applied())
    assert B.get_xfrc_applied()[1:5].any() and not B.get_xfrc_applied()[[0, 5]].any()
    A.step(2); B.step(2)
    _same(A, B, "xfrc_applied")
    x32b, x64b = _f32(rng, (NENV, m.nbody, 6), -20, 20)
    A.set_xfrc_applied(x64b); B.set_xfrc_applied_device(_dev(x32b))
    A.step(); B.step()
    _same(A, B, "xfrc_applied, second call")
    _close(A, B)


# ------------------------------------------------------------------ 3. joint-state read
def test_joint_state_rows_bitwise_with_guards(lib):
    m = fs.rig(lib)
    assert m.nv == 17 and m.nq != m.nv
    q, v, mocap = fs.states(m, NENV, slide=0.5)
    e = ms.Engine(m, NENV)
    e.set_state(qpos=q, qvel=v, time=np.zeros(NENV), warmstart=np.zeros_like(v))
    for k in range(m.nmocap):
        e.set_mocap_pose(k, mocap[:, k, :3], mocap[:, k, 3:])
    e.step(3, with_inverse=True)
    hq, hv, hf = e.get_joint_state()
    SENT, PAD = -7.25, 64

    def buf(rows, w):
        return torch.full((rows * w + PAD,), SENT, dtype=torch.float32, device="cuda")

    def check(t, want, rows, w, what):
        got = t.cpu().numpy()
        np.testing.assert_array_equal(got[:rows * w].reshape(rows, w), want.astype(np.float32), err_msg=what)
        assert (got[rows * w:] == SENT).all(), f"{what}: wrote past the end"

    bq, bv, bf = buf(NENV, m.nq), buf(NENV, m.nv), buf(NENV, m.nv)
    torch.cuda.synchronize()
    e.get_joint_state_device(bq.data_ptr(), bv.data_ptr(), bf.data_ptr())
    e.synchronize()
    check(bq, hq, NENV, m.nq, "qpos"); check(bv, hv, NENV, m.nv, "qvel"); check(bf, hf, NENV, m.nv, "qfrc_inverse")
    assert np.abs(hf).max() > 0
    # an output that is not asked for is not written; a sub-range writes its rows only
    bq, bv, bf = buf(2, m.nq), buf(2, m.nv), buf(2, m.nv)
    torch.cuda.synchronize()
    e.get_joint_state_device(None, bv.data_ptr(), None, env0=3, n=2)
    e.get_joint_state_device(bq[:2 * m.nq].view(2, m.nq), None, None, env0=3)      # n from the tensor's rows
    e.synchronize()
    check(bv, hv[3:5], 2, m.nv, "qvel rows 3, 4"); check(bq, hq[3:5], 2, m.nq, "qpos rows 3, 4")
    assert (bf.cpu().numpy() == SENT).all()
    e.close()


# ------------------------------------------------------------------ 4. masked reset
def _run_up(m, A, B, rng):
    """ten steps, then a split step left open with every field PH_RESET clears in use: qvel_ref and qfrc_applied stored by step1, a command
    pending for the next one"""
    c1, c1d = _f32(rng, (NENV, m.nv), -2, 2); c2, c2d = _f32(rng, (NENV, m.nv), -0.2, 0.2)
    for e in (A, B):
        e.step(10)
        e.set_cmd(c1d, c2d)
        e.step1()
        e.set_cmd(c2d, c1d * 0.1)
    return c1d


def _finish(A, B, what):
    _same(A, B, f"{what}: at once")
    A.step2(); B.step2()
    _same(A, B, f"{what}: after step2")
    A.step(5); B.step(5)
    _same(A, B, f"{what}: after five steps")


@pytest.mark.parametrize("name", ["s24", "arm7", "pile"])
def test_masked_reset(name):
    m, A, B = _twins(name)
    _run_up(m, A, B, np.random.default_rng(8))
    before = _snap(B)
    for i in IDS:
        A.reset([i])
    B.reset_device(_dev(MASK, torch.uint8))
    after = _snap(B)
    for i in range(NENV):      # the reset did something, and only where asked
        assert (after["time"][i] == 0) == bool(MASK[i]) and (before["time"][i] > 0)
        if not MASK[i]:
            np.testing.assert_array_equal(after["qpos"][i], before["qpos"][i])
    _finish(A, B, name)
    _close(A, B)


@pytest.mark.parametrize("name", ["s24", "arm7", "pile"])
def test_masked_reset_with_given_state(name):
    m, A, B = _twins(name)
    rng = np.random.default_rng(9)
    _run_up(m, A, B, rng)
    q0 = np.tile(m.array("qpos0"), (NENV, 1)).astype(np.float32)
    q32 = (q0 + rng.uniform(-0.01, 0.01, q0.shape)).astype(np.float32)      # as given: quaternions are not normalised
    v32, _ = _f32(rng, (NENV, m.nv), -0.3, 0.3)
    for i in IDS:
        A.reset([i])
        A.set_state(qpos=q32[i:i + 1].astype(np.float64), qvel=v32[i:i + 1].astype(np.float64), env0=i)
    hole = [i for i in range(NENV) if not MASK[i]]
    qb, vb = q32.copy(), v32.copy()
    qb[hole] = np.nan; vb[hole] = np.nan      # rows of envs that are not selected are never read
    B.reset_device(_dev(MASK, torch.bool), _dev(qb), _dev(vb))
    _finish(A, B, f"{name}, given qpos and qvel")
    # qvel alone: qpos from the initial qpos
    for i in IDS:
        A.reset([i])
        A.set_state(qvel=v32[i:i + 1].astype(np.float64), env0=i)
    B.reset_device(_dev(MASK, torch.uint8), None, _dev(vb))
    A.step(2); B.step(2)
    _same(A, B, f"{name}, given qvel")
    _close(A, B)


def test_reset_without_a_mask_is_the_range():
    m, A, B = _twins("s24")
    _run_up(m, A, B, np.random.default_rng(10))
    for i in (2, 3, 4):
        A.reset([i])
    B.reset_device(env0=2, n=3)
    _finish(A, B, "no mask, envs 2 .. 4")
    _close(A, B)


# ------------------------------------------------------------------ 5. mjh_reset with a list
def test_reset_with_an_id_list_is_the_single_id_calls():
    m, A, B = _twins("s24")
    _run_up(m, A, B, np.random.default_rng(11))
    for i in (4, 1, 4, 5):
        A.reset([i])
    B.reset([4, 1, 4, 5])
    _finish(A, B, "id list")
    for k in range(10):      # more calls than the ring of pinned slots has
        ids = [(k + 1) % NENV, (k + 3) % NENV]
        for i in ids:
            A.reset([i])
        B.reset(ids)
        A.step(); B.step()
    _same(A, B, "ten lists")
    with pytest.raises(ms.engine.MjhError, match="out of range"):
        B.reset([1, NENV])
    _same(A, B, "a refused list resets nothing")
    _close(A, B)


# ------------------------------------------------------------------ 6. reporting engine
def test_masked_reset_clears_the_selected_envs_report(lib):
    nenv = 4
    m = cs.arm_scene(lib); q, v, xf = cs.arm_states(m, nenv)
    e = ms.Engine(m, nenv, contact_report=True)
    e.set_state(qpos=q, qvel=v, time=np.zeros(nenv), warmstart=np.zeros_like(v)); e.set_xfrc_applied(xf)
    e.step(3)
    info = e.contact_report_device()
    hip = C.CDLL("libamdhip64.so")

    def raw():
        e.synchronize()
        r = np.zeros((nenv, info["maxcon"], 20), dtype=np.float32)
        assert hip.hipMemcpy(r.ctypes.data_as(C.c_void_p), C.c_void_p(info["records"]), C.c_size_t(r.nbytes), 2) == 0
        return r

    rep, ext, rec = e.contact_forces(), e.cfrc_ext(), raw()
    assert (rep["ncon"] > 0).all() and all(ext[i].any() and rec[i].any() for i in range(nenv))
    e.reset_device(_dev([0, 1, 1, 0], torch.uint8))
    rep2, ext2, rec2 = e.contact_forces(), e.cfrc_ext(), raw()
    for i in (1, 2):
        assert rep2["ncon"][i] == 0 and not ext2[i].any() and not rec2[i].any()
    for i in (0, 3):
        assert rep2["ncon"][i] == rep["ncon"][i]
        np.testing.assert_array_equal(rec2[i], rec[i]); np.testing.assert_array_equal(ext2[i], ext[i])
    e.close()


# ------------------------------------------------------------------ 7. cohorts
def test_forked_cohorts():
    nenv = 128
    m, A, B = _twins("s24", nenv)
    rng = np.random.default_rng(12)
    for e in (A, B):
        e.set_cohorts(2)
        e.step(2)      # the cohort streams are forked from here on
    a32, a64 = _f32(rng, (10, m.nv), -3, 3); b32, b64 = _f32(rng, (10, m.nv), -0.2, 0.2)
    da, db = _dev(a32), _dev(b32)
    A.set_cmd(a64, b64, env0=70); B.set_cmd_device(da, db, env0=70)      # inside the second cohort
    gq = torch.zeros(10, m.nq, dtype=torch.float32, device="cuda"); torch.cuda.synchronize()
    B.get_joint_state_device(gq, env0=70)      # read on that cohort's stream
    A.set_cmd(b64, a64 * 0.1, env0=60); B.set_cmd_device(db, _dev((a64 * 0.1).astype(np.float32)), env0=60)      # across both
    gv = torch.zeros(10, m.nv, dtype=torch.float32, device="cuda"); torch.cuda.synchronize()
    B.get_joint_state_device(qvel=gv, env0=60)      # across both: each cohort writes its rows
    B.synchronize()
    np.testing.assert_array_equal(gq.cpu().numpy(), A.get_joint_state(70, 10)[0].astype(np.float32))
    np.testing.assert_array_equal(gv.cpu().numpy(), A.get_joint_state(60, 10)[1].astype(np.float32))
    assert gv.cpu().numpy()[[0, 3, 4, 9]].any(axis=1).all()
    mask = (rng.uniform(size=nenv) < 0.3).astype(np.uint8); mask[[0, 63, 64, 127]] = 1
    for i in np.flatnonzero(mask):
        A.reset([int(i)])
    B.reset_device(_dev(mask, torch.uint8))
    A.step(3); B.step(3)
    _same(A, B, "cohorts")
    # once more with the streams forked when the reset arrives
    mask2 = (rng.uniform(size=40) < 0.5).astype(np.uint8)
    for i in np.flatnonzero(mask2):
        A.reset([50 + int(i)])
    B.reset_device(_dev(mask2, torch.uint8), env0=50)
    A.step(); B.step()
    _same(A, B, "cohorts, reset while forked")
    _close(A, B)


# ------------------------------------------------------------------ 8. stream order
def test_closed_loop_in_stream_order_without_synchronisation():
    kd = np.float32(0.75)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        m, A, B = _twins("arm7", stream=torch.cuda.current_stream().cuda_stream)
        assert torch.cuda.current_stream().cuda_stream == side.cuda_stream
        qv = torch.zeros(NENV, m.nv, dtype=torch.float32, device="cuda")
        for _ in range(20):
            B.get_joint_state_device(qvel=qv)
            ddq = qv * (-kd)      # one multiply, exact in fp32; a new buffer every iteration, released in stream order
            B.set_cmd_device(ddq)
            B.step()
        for _ in range(20):
            v = A.get_joint_state()[1].astype(np.float32)
            A.set_cmd((v * (-kd)).astype(np.float64))
            A.step()
        _same(A, B, "closed loop")
        _close(A, B)
