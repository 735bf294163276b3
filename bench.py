#!/usr/bin/env python
"""bench.py — env-steps/sec of the BASELINE.json configs on N MI355X (default: S24, the metric's scene).

A "step" is one pass of the hot path — mj_step1 + controller + [mj_inverse] + mj_step2 (reference loop body,
src/mj_main.cpp:82-112) — over one batch of environments per GPU, one launch per step and cohort (the drop-in keeps the
reference's per-step host hand-off to ros_control).  Inputs are resident in HBM when the timed region starts.

    python bench.py --gpus N --steps K --warmup W [--config s24|c2|c3|c4|c5] [--dump-outputs DIR] [--full]

Every config first runs its FIXED, untimed settle phase (S24 400 steps, C2 200, ...) — independent
of --warmup — so that the timed window always steps the scene the metric names; then W untimed warm-up steps, then EXACTLY K
timed steps bracketed by barrier + synchronize.  N > 1: launched by torch.distributed.run, one rank per GPU; environments
are sharded (rank r owns envs [r*n, (r+1)*n)), no data-path collective; the only collective is the RCCL all-gather of the
published state slice at 60 Hz of simulated time, packed (mjh_export_state_device) at that rate at every N
so that per-GPU work does not depend on N.  Prints ONE JSON line on rank 0.

A plain run does only what the headline needs: set-up, settle, warm-up, the K timed steps, the line.  --full adds what takes runs
of its own: the second timed window (the other mj_inverse variant), the CPU baseline, and for S24 at N = 1 the literal reference
loop and the other BASELINE configs, each in a process of its own (--no-second-window / --no-cpu-baseline / --no-extra-configs
drop one of them again).  --dump-outputs DIR writes the state the timed path leaves after its last step (what mjh_get_state and
mjh_get_stats hand a caller), per environment, as DIR/<name>.npy in float64: the inputs are seeded, so two builds run with the
same arguments can be compared array for array.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# The engine steps two or three env cohorts on their own HIP streams; with RCCL's streams on top, more than the default 4
# hardware queues are in use and streams that share a queue serialise (measured: 4.19 M vs 4.73 M env-steps/s on the
# publish path).  Must be set before the HIP runtime initialises, i.e. before torch is imported.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (~6.3 TB/s achievable)
METRIC = "env-steps/sec (whole node) at 4096 envs, 24-DoF/30-contact scene; 1/2/4/8 GPUs"
GOLD = os.path.join(ROOT, "tests", "golden")


def algorithmic_bytes_per_env_step(nq, nv):
    """read qpos,qvel,warmstart,cmd(ddq,dq); write qpos,qvel,warmstart; fp32."""
    return 4 * (2 * nq + 6 * nv)


def robot_command(m, k):
    """commanded joint accelerations of the robot fixtures (same generator as tests/test_robot_fixtures.py)"""
    jt = m.array("jnt_type"); da = m.array("jnt_dofadr")
    ddq = np.zeros(m.nv)
    for j in range(m.njnt):
        if jt[j] in (2, 3):
            ddq[da[j]] = 0.8 * np.sin(0.05 * k + 0.37 * j)
    return ddq


class Workload:
    """One BASELINE.json config as concrete inputs.  `inverse` = the ros_control read path
    (mj_inverse every step, mj_hw_interface.cpp:61): the robot configs always pay it, as the reference does."""
    name = ""; label = ""; envs_per_gpu = 4096; settle_steps = 0; inverse = False; min_ncon = None

    pack = 1          # environments per wavefront (mjh_model_replicate: sub-wave packing of small models); 1 = one wave per env
    cohorts = 0       # env cohorts on separate HIP streams; 0 = the engine's default (two for a fused step, three for the many-body layout)

    def __init__(self, ms, args, rank, device, stream):
        self.ms = ms; self.args = args; self.rank = rank
        self.nenv = args.envs_per_gpu or self.envs_per_gpu          # ENVIRONMENTS per GPU
        if args.pack > 0:
            self.pack = args.pack
        if self.nenv % self.pack:
            raise SystemExit(f"--envs-per-gpu {self.nenv} is not a multiple of the {self.pack} environments per wavefront")
        self.rows = self.nenv // self.pack                          # engine rows = wavefronts
        self.env_offset = rank * self.nenv
        self.tab = None; self.step_count = 0
        self.build(device, stream)
        if not hasattr(self, "base_model"):
            self.base_model = self.model                            # the single-environment model (oracle, byte accounting)

    def packed(self, base):
        """the model the engine steps: `pack` independent instances of `base` per wavefront (row w = envs w*pack .. w*pack+pack-1)"""
        self.base_model = base
        return base.replicate(self.pack) if self.pack > 1 else base

    def env_state(self, n):
        """(qpos, qvel, warmstart, stats) of the first n ENVIRONMENTS"""
        rows = -(-n // self.pack)
        _, q, v, ws = self.eng.get_state(0, rows); st = self.eng.get_stats(0, rows)
        bq, bv = self.base_model.nq, self.base_model.nv
        st = np.repeat(st.astype(np.float64), self.pack, axis=0)[:n]
        st[:, :2] /= self.pack                                       # (a wavefront's contact / row counts cover its `pack` environments)
        return q.reshape(rows * self.pack, bq)[:n], v.reshape(rows * self.pack, bv)[:n], ws.reshape(rows * self.pack, bv)[:n], st

    # -- hooks
    def build(self, device, stream): raise NotImplementedError
    def before_step(self, k): pass                     # host-side work of step k of the run (service calls, new targets)
    def oracle_data(self, orc, i, state): raise NotImplementedError
    def extra_config(self): return {}

    def quiet_steps(self, k):
        """steps from step k on (k included) that need no host-side work between them: 1 unless a config knows its schedule"""
        return 1 << 30 if type(self).before_step is Workload.before_step else 1

    def step(self, n, inverse):
        # one mjh_step call per stretch without host work: the engine turns it into one launch per cohort where its kernel carries the
        # step loop (steps_per_launch), into back-to-back launches elsewhere
        while n > 0:
            self.before_step(self.step_count)
            k = max(1, min(n, self.quiet_steps(self.step_count)))
            self.eng.step(k, inverse)
            self.step_count += k; n -= k


class S24(Workload):
    name = "s24"; settle_steps = 400; min_ncon = 8.0
    cohorts = 3       # 9.49 / 9.80 / 9.24 M env-steps/s with 2 / 3 / 4 cohorts (the third fills the tails of the other two; the engine's own default for a fused step is 2)
    label = "S24: 4 free boxes (24 DoF) in a walled pen on the empty.xml floor, PGS 100 it / tol 1e-8"

    def build(self, device, stream):
        self.model = self.ms.scene("s24")
        if self.args.maxcon > 0:
            self.model.c.maxcon = self.args.maxcon; self.model.c.maxefc = 6 * self.args.maxcon
        self.eng = self.ms.Engine(self.model, self.nenv, device=device, stream=stream)
        self.tab = self.eng.load_s24(env_offset=self.env_offset)

    def oracle_data(self, orc, i, state):
        from mujoco_sim_amd.engine import EP
        d = orc.OrcData(self.model.ptr)
        for k, wh in EP.items():
            d.set_env_param(wh, self.tab[k][i])
        return d

    def extra_config(self):
        # "the harness must print the measured ncon / nefc so the ~30 claim is checked, not assumed"
        st = self.eng.get_stats()
        hc, _ = np.histogram(st[:, 0], bins=[0, 8, 16, 24, 32, 40, 48, 64, 100000])
        hr, _ = np.histogram(st[:, 1], bins=[0, 33, 65, 97, 129, 161, 193, 209, 257, 321, 100000])
        return {"ncon_histogram": dict(zip(["0-7", "8-15", "16-23", "24-31", "32-39", "40-47", "48-63", "64+"], map(int, hc))),
                "nefc_histogram": dict(zip(["0-32", "33-64", "65-96", "97-128", "129-160", "161-192", "193-208", "209-256", "257-320", "321+"], map(int, hr)))}


class S24D(S24):
    cohorts = 3       # round 6 (32-row section off, 64-row form above 192 rows): 6.19 / 6.28 / 5.83 M env-steps/s on 2 / 3 / 4 cohorts (round 5, section on, threshold 208: 5.75 / 5.56 M on 2 / 3)
    """the "30-contact" reading of the metric's name: S24's pen and S24's four boxes (same per-env sizes, masses, seeds), but released
    flat and side by side (2 x 2, random yaw) instead of as a staggered column of random orientations: the boxes land on the floor
    together (16 floor contacts of condim 4) and are wedged against each other and the walls — ~30 contacts, ~130 rows per env, what
    SURVEY.md §8-d D2 expected of the scene.  Reported beside the D2-exact S24 line, never instead of it."""
    name = "s24d"; settle_steps = 400; min_ncon = 20.0
    pen_half = 0.175; capacity = 96      # (piles reach 68 contacts / 300 rows: tools/r05_hist.py; up to 64 the model keeps the contact-patch sweep as well)
    label = ("S24D: S24's pen and 4 free boxes (same sizes / seeds), released flat in a 2 x 2 layout with random yaw: ~30 contacts, ~130 rows per env, "
             "PGS 100 it / tol 1e-8")

    def build(self, device, stream):
        mc = self.args.maxcon if self.args.maxcon > 0 else self.capacity
        pen = float(self.args.pen_half or self.pen_half)
        self.model = self.ms.scene("s24pen", pen, int(mc))
        self.eng = self.ms.Engine(self.model, self.nenv, device=device, stream=stream)
        self.tab = self.eng.load_s24(env_offset=self.env_offset)
        q = self.tab["qpos"].reshape(self.nenv, 4, 7)
        for i in range(self.nenv):
            rng = np.random.default_rng(0x524D0000 + self.env_offset + i)
            for k in range(4):
                yaw = rng.uniform(-0.3, 0.3)
                q[i, k] = [(-1 if k & 1 else 1) * pen / 2, (-1 if k & 2 else 1) * pen / 2, 0.16 + 0.02 * k, np.cos(yaw / 2), 0, 0, np.sin(yaw / 2)]
        self.eng.set_initial_qpos(self.tab["qpos"]); self.eng.reset()

    def oracle_data(self, orc, i, state):
        d = super().oracle_data(orc, i, state)
        return d


class C2(S24):
    name = "c2"; settle_steps = 200; min_ncon = None
    cohorts = 4       # round 5: 0.477 - 0.478 M on four cohorts against 0.470 - 0.472 M on three (two same-call A/Bs)
    label = ("C2: 64 free boxes (nv 384), half-extents U[0.05,0.125]^3, 4x4x4 lattice (pitch 0.3 m, z0 0.5..1.4) with +-0.01 m jitter and "
             "random orientation, on the empty.xml floor")

    def build(self, device, stream):
        self.model = self.ms.scene("boxpile", 64)
        mc = self.args.maxcon if self.args.maxcon > 0 else 600
        self.model.c.maxcon = mc; self.model.c.maxefc = 4 * mc
        self.eng = self.ms.Engine(self.model, self.nenv, device=device, stream=stream)
        self.tab = self.eng.load_tables(self.ms.boxes_randomize(self.model, self.env_offset, self.nenv, jitter=0.01))

    def extra_config(self):
        st = self.eng.get_stats()
        hist, edges = np.histogram(st[:, 0], bins=[0, 64, 128, 192, 256, 320, 384, 448, 512, 100000])
        return {"ncon_histogram": {f"{int(edges[i])}-{int(edges[i + 1]) - 1}" if i < 8 else "512+": int(hist[i]) for i in range(9)}}


class C3(Workload):
    name = "c3"; envs_per_gpu = 8192; settle_steps = 200; inverse = True
    label = ("C3: 7-hinge Panda chain (limits of ridgeback_panda.xml:53-87), fixed base, gravcomp 1, computed-torque wrapper + mj_inverse, "
             "PD ddq = 200 (q* - q) - 50 qd in the engine, targets U[limits] re-drawn every 200 steps; four arms per wavefront (mjh_model_replicate)")

    pack = 4          # four arms per wavefront (7 of 64 lanes busy otherwise): mjh_model_replicate, HISTORY.md §9
    cohorts = 2       # round 5, with all 2048 workgroups resident (16 LDS granules): 101.4 - 101.7 M on two cohorts against 99.7 - 99.9 M on three, three same-call A/Bs (round 4: 74 / 79 M with 2 / 3 cohorts; four: 54 M, the per-step join for the publish copy costs more than the overlap gives; tools/c3_sweep.sh)

    def build(self, device, stream):
        self.model = self.packed(self.ms.scene("arm7", 1))
        self.eng = self.ms.Engine(self.model, self.rows, device=device, stream=stream)
        self.eng.set_controlled_dofs(np.ones(self.model.nv, dtype=np.int32))
        self.rng = np.random.default_rng(0xC3 + self.rank)
        self.lo, self.hi = self.base_model.array("jnt_range").reshape(-1, 2).T
        self.eng.set_pd_controller(200.0, 50.0)          # box.yaml:8 (integral term dropped, as SURVEY §8-d D3 states)
        self.target = None

    def before_step(self, k):
        if k % 200 == 0:
            self.target = self.rng.uniform(self.lo, self.hi, size=(self.nenv, self.base_model.nv))
            self.eng.set_pd_target(self.target.reshape(self.rows, -1))

    def quiet_steps(self, k):
        return 200 - k % 200

    def oracle_data(self, orc, i, state):
        d = orc.OrcData(self.base_model.ptr)
        d.ifield("controlled")[:] = 1
        d.set_pd(self.target[i], 200.0, 50.0)
        return d


class RobotFixture(Workload):
    fixture = ""; inverse = True

    def build(self, device, stream):
        from mujoco_sim_amd.tables import load_model_tables
        base, self.z = load_model_tables(os.path.join(GOLD, f"robot_{self.fixture}.npz"))
        self.model = self.packed(base)
        self.eng = self.ms.Engine(self.model, self.rows, device=device, stream=stream)
        self.controlled = self.z["controlled"].astype(np.int32)
        self.eng.set_controlled_dofs(np.tile(self.controlled, self.pack))

    def oracle_data(self, orc, i, state):
        d = orc.OrcData(self.base_model.ptr)
        d.ifield("controlled")[:] = self.controlled
        return d


class C4(RobotFixture):
    name = "c4"; envs_per_gpu = 2048; settle_steps = 200; fixture = "c4_pr2_world_objects_mesh"
    label = ("C4: PR2 (nv 49, 6 joint equalities, 37 mesh geoms as convex hulls) on the reference floor + pool of 8 spawnable objects in one "
             "model, computed-torque wrapper + mj_inverse, every 100 steps 1/16 of the envs get one object spawned and one destroyed")

    def build(self, device, stream):
        super().build(device, stream)
        lib = self.ms.capi.load()
        names = [lib.mjh_id2name(self.model.ptr, 0, b).decode() for b in range(self.model.c.nbody)]
        self.slots = [b for b, n in enumerate(names) if n.startswith("object_")]
        for b in self.slots:
            self.eng.set_slot_active(b, False)                      # the pool starts empty
        self.active = np.zeros((self.nenv, len(self.slots)), dtype=bool)
        self.rng = np.random.default_rng(0xC4 + self.rank)
        self.service_s = 0.0; self.service_calls = 0

    def churn(self):
        """spawn_objects / destroy_objects (mj_ros.cpp:859-1507) as slot toggles + initial pose and twist (mj_ros.cpp:1406-1412)"""
        self.eng.synchronize()            # (so that the service time below is the calls', not the drain of the queued steps)
        t0 = time.perf_counter()
        senv, sbody, spos, denv, dbody = [], [], [], [], []
        for i in self.rng.choice(self.nenv, max(1, self.nenv // 16), replace=False):
            off = np.nonzero(~self.active[i])[0]; on = np.nonzero(self.active[i])[0]
            if len(on) > 2:
                k = int(self.rng.choice(on)); denv.append(int(i)); dbody.append(self.slots[k]); self.active[i, k] = False
            if len(off):
                k = int(self.rng.choice(off)); a = self.rng.uniform(-np.pi, np.pi); r = self.rng.uniform(0.8, 1.5)
                senv.append(int(i)); sbody.append(self.slots[k]); spos.append([r * np.sin(a), r * np.cos(a), 2.0]); self.active[i, k] = True
        # one service call each, as the reference's services take lists of objects (mj_ros.cpp:859-904,1430-1507)
        if denv:
            self.eng.destroy_objects(denv, dbody)
        if senv:
            self.eng.spawn_objects(senv, sbody, np.array(spos))
        self.service_s += time.perf_counter() - t0; self.service_calls += 1

    def before_step(self, k):
        if k < self.settle_steps:
            if k % 25 == 24:
                self.churn()                                        # fill the pools a little while settling
            if k % 10 == 0:
                self.eng.set_cmd(ddq=np.tile(robot_command(self.model, k), (self.nenv, 1)))
        elif (k - self.settle_steps) % 100 == 0:
            self.churn()

    def oracle_data(self, orc, i, state):
        d = super().oracle_data(orc, i, state)
        sbase = self.model.c.nbody - 32 if self.model.c.nbody > 32 else 0
        mask = 0
        for k, b in enumerate(self.slots):
            if not self.active[i, k]:
                mask |= 1 << (b - sbase)
        orc.lib().orc_set_slot_mask(d.d, mask)
        return d

    def extra_config(self):
        return {"objects_alive_per_env": float(self.active.sum(1).mean()),
                "service_ms_per_churn": 1e3 * self.service_s / max(self.service_calls, 1), "churns": self.service_calls}


class C5(RobotFixture):
    name = "c5"; envs_per_gpu = 4096; settle_steps = 100; fixture = "c5_pendulum_bowl_mesh"
    label = ("C5: multi_mujoco_sim.launch scene (pendulum.xml world + static bowl.xml, 37 mesh geoms), 32768 envs over 8 GPUs = 4096 per GPU, "
             "mj_inverse every step, state all-gather at 60 Hz")

    # (packing two worlds per wavefront — `--pack 2`, the static bowl shared — changes nothing at 4096 envs per GPU: 32.8 M
    # against 33.0 M env-steps/s, the step is bound by its ~6 launches, not by the kernels)

    def build(self, device, stream):
        super().build(device, stream)
        rng = np.random.default_rng(0xC5 + self.rank)
        if "qvel0" in self.z and np.any(self.z["qvel0"]):      # per-env spin so that the envs differ
            v = self.z["qvel0"][None, :] * rng.uniform(0.5, 1.5, size=(self.nenv, 1))
            self.eng.set_state(qvel=v.reshape(self.rows, -1))


WORKLOADS = {w.name: w for w in (S24, S24D, C2, C3, C4, C5)}


def usable_cpus():
    """CPUs this process may actually run on: the scheduler affinity mask, capped by the cgroup CPU quota (v2 cpu.max, v1
    cfs_quota / cfs_period) — os.cpu_count() reports the machine, not the container."""
    info = {"os_cpu_count": os.cpu_count() or 1}
    try:
        aff = len(os.sched_getaffinity(0))
    except Exception:
        aff = info["os_cpu_count"]
    info["sched_affinity"] = aff
    quota = None
    try:
        t = open("/sys/fs/cgroup/cpu.max").read().split()
        if t and t[0] != "max":
            quota = float(t[0]) / float(t[1])
        info["cgroup_cpu_max"] = " ".join(t)
    except Exception:
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read()); p = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / p
            info["cgroup_cfs_quota_over_period"] = q / p if q > 0 else "unlimited"
        except Exception:
            pass
    n = aff if quota is None else max(1, min(aff, int(quota + 0.5)))
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                info["cpu_model"] = line.split(":", 1)[1].strip(); break
    except Exception:
        pass
    info["usable"] = n
    return n, info


def cpu_baseline(w, sample_envs, budget_s, with_inverse):
    """Oracle (fp64 C restatement, test infrastructure) timed on the host cores on a bounded sample of the SAME workload:
    the first envs of the run, started from the state the GPU holds when the timed window ends.  Thread scaling 1 / 8 / 64 /
    all usable cores, every point after a warm pass; `value` is the all-cores point, `cores` the threads it used."""
    import ctypes as C
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import orc

    L = orc.lib()
    ncores, cpuinfo = usable_cpus()
    sample_envs = min(sample_envs, w.nenv)
    q, v, ws, st = w.env_state(sample_envs)
    ds = []

    def ensure(n):                                   # oracle data of the first n sample envs (created on demand: C2's are large)
        for i in range(len(ds), n):
            d = w.oracle_data(orc, i, None)
            d.set_qpos(q[i]); d.f("qvel")[:] = v[i]; d.f("qacc_warmstart")[:] = ws[i]; d.f("qacc")[:] = ws[i]
            ds.append(d)
        return (C.c_void_p * n)(*[d.d for d in ds[:n]])

    points = sorted({t for t in (1, 8, 64, ncores) if t <= ncores})
    per_point = budget_s / len(points)
    table = []
    for T in points:
        L.orc_set_threads(T)
        ncal = min(sample_envs, T)
        arr = ensure(ncal)
        L.orc_step_many(arr, ncal, 1, int(with_inverse))                 # (creates the team's threads, faults the data in)
        cal = max(min(L.orc_step_many_timed(arr, ncal, 1, 1, int(with_inverse)) for _ in range(3)), 1e-6)   # one env-step per thread (the fastest of three: one slow sample on a shared host would shrink the whole point's sample)
        afford = per_point * T / cal                  # env-steps this point can afford
        n_envs = min(sample_envs, max(T, min(max(4 * T, 64), int(afford // 4))))
        n_steps = max(1, min(200, int(afford // n_envs)))
        arr = ensure(n_envs)
        # warm step and timed steps inside ONE parallel region: the clock starts with every thread awake (orc_step_many_timed)
        # (twice, the faster one counts: shared hosts are noisy — a run can lose half its threads to a neighbour)
        n_steps = max(1, n_steps // 2)
        if T == 1:
            n_steps = max(n_steps, -(-256 // n_envs))     # the 1-thread figure rests on >= 256 env-steps whatever a loaded host's calibration said
        runs = [L.orc_step_many_timed(arr, n_envs, 1, n_steps, int(with_inverse)) for _ in range(2)]
        dt = min(runs)
        table.append({"threads": T, "value": n_envs * n_steps / dt, "envs": n_envs, "steps": n_steps, "seconds": dt, "seconds_each_run": runs})
    one, top = table[0], table[-1]
    for r in table:
        r["speedup_vs_1thread"] = r["value"] / one["value"]
    nefc = float(np.mean([d.i("nefc") for d in ds])); ncon = float(np.mean([d.i("ncon") for d in ds]))
    n = len(ds)
    return {
        "value": top["value"], "unit": "env-steps/s", "cores": top["threads"], "kind": "port",
        "value_1thread": one["value"], "env_steps_1thread": one["envs"] * one["steps"], "scaling": table, "host": cpuinfo,
        "mean_nefc": nefc, "mean_ncon": ncon,
        "gpu_mean_nefc_same_envs": float(st[:n, 1].mean()), "gpu_mean_ncon_same_envs": float(st[:n, 0].mean()),
        "with_inverse": bool(with_inverse),
        "sample": f"oracle/ fp64 C restatement (PGS in MuJoCo's dense-AR form; no allocation inside a step), the first {top['envs']} {w.name} envs started from the "
                  f"GPU's state at the end of the timed window, {top['steps']} steps after a warm step (best of two runs), a team of {top['threads']} spinning threads drawing (env, 4-step) items = "
                  f"the usable cores (affinity {cpuinfo['sched_affinity']}, os.cpu_count {cpuinfo['os_cpu_count']}, cgroup quota {cpuinfo.get('cgroup_cpu_max', cpuinfo.get('cgroup_cfs_quota_over_period', 'n/a'))}); "
                  f"1-thread figure: {one['steps']} steps of {one['envs']} envs (the reference itself steps on one thread, mj_main.cpp:203); "
                  f"reference library (libmujoco 2.3.7) absent from this image",
    }


def launcher_command(argv, ngpus, port=None):
    """argv of the one-rank-per-GPU launch of this script (what the driver runs for N > 1)"""
    if port is None:
        import socket
        sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    return [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={ngpus}", "--master-addr", "127.0.0.1",
            "--master-port", str(port), os.path.abspath(__file__)] + list(argv)


def relaunch_under_torchrun(args):
    """`python bench.py --gpus N` invoked plainly (no WORLD_SIZE): become the N-rank launch instead of refusing."""
    cmd = launcher_command(sys.argv[1:], args.gpus)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    sys.stdout.flush(); sys.stderr.flush()
    os.execv(sys.executable, cmd)


def run_group_host(args):
    """--host group: ONE process drives every GPU through the C host API (mjh_group_*: one engine + stream per device, one
    host thread, RCCL ncclAllGather of the published slice) — the shape of the reference's single node (mj_main.cpp:167-236,
    one publisher set mj_ros.cpp:554-564; launch/multi_mujoco_sim.launch:9-34 for config C5).  Needs no launcher."""
    import ctypes as C

    import mujoco_sim_amd as ms

    if args.config not in ("s24", "c5"):
        raise SystemExit("--host group runs the configs whose environments need no per-step host work: s24, c5")
    devices = [int(x) for x in args.group_devices.split(",")] if args.group_devices else list(range(args.gpus))
    ndev = len(devices)
    wcls = WORKLOADS[args.config]
    per_gpu = args.envs_per_gpu or wcls.envs_per_gpu
    total = per_gpu * ndev
    if args.config == "s24":
        model = ms.scene("s24"); z = None
    else:
        from mujoco_sim_amd.tables import load_model_tables
        model, z = load_model_tables(os.path.join(GOLD, f"robot_{wcls.fixture}.npz"))
    g = ms.Group(model, total, devices)
    for k, (lo, n) in enumerate(g.ranges):
        e = g.engines[k]
        if args.cohorts > 0 or wcls.cohorts > 0:
            e.set_cohorts(args.cohorts if args.cohorts > 0 else wcls.cohorts)
        if args.config == "s24":
            e.load_s24(env_offset=lo)
        else:
            e.set_controlled_dofs(z["controlled"].astype(np.int32))
            if "qvel0" in z and np.any(z["qvel0"]):
                rng = np.random.default_rng(0xC5 + k)
                e.set_state(qvel=z["qvel0"][None, :] * rng.uniform(0.5, 1.5, size=(n, 1)))
    inverse = wcls.inverse if args.with_inverse < 0 else bool(args.with_inverse)
    publish_every = max(1, int(round(1.0 / (60.0 * model.opt.timestep))))
    count = [0]
    issue = {"step_s": 0.0, "step_calls": 0, "publish_s": 0.0, "publish_calls": 0}     # wall time the ONE host thread spends inside the calls
    if args.steps_per_launch > 0:
        for e in g.engines:
            e.set_steps_per_launch(args.steps_per_launch)

    def run(nsteps):
        while nsteps > 0:
            k = nsteps if args.no_gather else min(nsteps, publish_every - count[0] % publish_every)
            t_ = time.perf_counter(); g.step(k, inverse); issue["step_s"] += time.perf_counter() - t_; issue["step_calls"] += 1
            count[0] += k; nsteps -= k
            if not args.no_gather and count[0] % publish_every == 0:
                t_ = time.perf_counter(); g.publish_device(); issue["publish_s"] += time.perf_counter() - t_; issue["publish_calls"] += 1

    run(wcls.settle_steps); run(args.warmup); g.synchronize()
    g.engines[0].set_launch_timing(max(1, args.timing_stride))
    for k_ in issue:
        issue[k_] = 0
    t0 = time.perf_counter(); run(args.steps); t_issued = time.perf_counter() - t0; g.synchronize(); elapsed = time.perf_counter() - t0
    kernel_ms, n_timed = g.engines[0].get_launch_timing(); g.engines[0].set_launch_timing(False)
    issue_timed = dict(issue)
    if args.dump_outputs:
        states = [e.get_state() for e in g.engines]
        save_outputs(args.dump_outputs, {"time": np.concatenate([x[0] for x in states]), "qpos": np.concatenate([x[1] for x in states]),
                                         "qvel": np.concatenate([x[2] for x in states]), "qacc_warmstart": np.concatenate([x[3] for x in states]),
                                         "stats": np.concatenate([e.get_stats().astype(np.float64) for e in g.engines]),
                                         "env_ids": np.concatenate([np.arange(lo, lo + n, dtype=np.float64) for lo, n in g.ranges])})
    # the exchange's own duration: a second, short window (reading the event pair of the previous publish makes the host wait for it —
    # kept out of the timed window, whose host time is the issue time reported below)
    g.set_publish_timing(True); run(min(args.steps, 20 * publish_every)); g.synchronize()
    ag_ms, ag_n = g.get_publish_timing(); g.set_publish_timing(False)
    issue = issue_timed
    st = np.concatenate([e.get_stats() for e in g.engines])
    cohorts = g.engines[0].cohorts
    G = cohorts if (cohorts > 1 and g.ranges[0][1] >= 64 * cohorts) else 1
    bytes_step = algorithmic_bytes_per_env_step(model.nq, model.nv)
    envs_per_launch = g.ranges[0][1] / G
    spl = int(g.engines[0].steps_per_launch) if args.no_gather else min(int(g.engines[0].steps_per_launch), publish_every)
    achieved = bytes_step * envs_per_launch * spl / (kernel_ms * 1e-3) / 1e9 if kernel_ms > 0 else 0.0
    # one host thread issues every device's launches (csrc/group.hip): if the time it spends inside the calls reaches the wall time of
    # the window, the group host — not the devices — sets the rate (measurable on one device: --group-devices 0,0,0,0,0,0,0,0)
    host_issue = {"ms_per_step_in_mjh_group_step": 1e3 * issue["step_s"] / args.steps, "ms_per_publish_call": 1e3 * issue["publish_s"] / max(issue["publish_calls"], 1),
                  "issue_fraction_of_wall": (issue["step_s"] + issue["publish_s"]) / elapsed, "wall_ms_until_everything_was_issued": 1e3 * t_issued,
                  "launches_per_step": ndev * G / spl, "steps_per_launch": spl}
    out = {
        "metric": METRIC if args.config == "s24" else f"env-steps/sec (whole node), BASELINE config {args.config.upper()}",
        "value": total * args.steps / elapsed, "unit": "env-steps/s", "n_gpus": ndev, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f32", "data": "synthetic",
        "config": {"workload": wcls.label, "name": args.config, "settle_steps": wcls.settle_steps, "envs_per_gpu": per_gpu, "envs_total": total,
                   "cohorts": cohorts, "steps_per_launch": spl, "with_inverse": bool(inverse), "parallelism": f"env-sharded x{ndev}, one process (mjh_group)",
                   "nq": int(model.nq), "nv": int(model.nv), "mean_ncon": float(st[:, 0].mean()), "mean_nefc": float(st[:, 1].mean()),
                   "mean_solver_iter": float(st[:, 2].mean())},
        "host": {"kind": "group", "api": "mjh_group_create / mjh_group_step / mjh_group_publish (csrc/group.hip)", "devices": devices,
                 "ranks": [{"rank": k, "device": devices[k], "env0": lo, "nenv": n} for k, (lo, n) in enumerate(g.ranges)],
                 "host_issue": host_issue, "host_threads": int(ms.capi.load().mjh_group_host_threads(g.h)), "rccl": bool(g.uses_rccl), "rccl_ranks": ndev if g.uses_rccl else 0,
                 "transport": "RCCL ncclAllGather (ncclCommInitAll; every device's host thread enqueues its own rank)" if g.uses_rccl else "peer copies (hipMemcpyPeerAsync)",
                 "all_gather": {"ms_mean": ag_ms, "count": ag_n, "bytes_per_rank": int(g.ranges[0][1] * g.stride * 4), "publish_every_steps": publish_every}},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": None,
                     "kernel": "mjh_step_kernel", "kernel_ms": kernel_ms, "launches_timed": n_timed, "envs_per_launch": envs_per_launch,
                     "algorithmic_bytes_per_env_step": bytes_step, "note": "device 0's launches; per-launch figure"},
    }
    g.close()
    try:
        C.CDLL(None).fflush(None)
    except Exception:
        pass
    print(json.dumps(out), flush=True)


# Timed windows of the configs that ride in the driver's line (settle phases are the workloads' own): (warm-up, timed steps).
# Fixed — NOT --steps — so that the driver's short command measures each config over the window its stand-alone profile run uses
# (VERDICT r05 #5, #9): C2 200 settle + 500 timed as D3 states it; C4 three spawn / destroy rounds; C3 / C5 at a fixed offset in simulated time
# (C5: more pendulums reach the bowl as time goes on); S24D 200 steps (six renewals of the launch order).
EXTRA_WINDOWS = {"s24d": (20, 200), "c2": (5, 500), "c3": (20, 300), "c4": (5, 300), "c5": (20, 300), "s24": (20, 100)}


def child_config_line(args, name, pgs=1):
    """One of the other BASELINE configs under the driver's fixed command, as a PROCESS OF ITS OWN running this script stand-alone
    (`--config name`, the config's D3 window, no CPU leg): the same streams in the same creation order, the same hardware queues, the same
    numbers as the stand-alone profile runs under profiles/ — inside the S24 process, behind its three cohort streams, S24D read 15 % low
    (BENCH_r05: 4.76 M against 5.6 - 5.8 M stand-alone; streams map onto the hardware queues in creation order, HISTORY.md Round 5).
    Returns the child's line condensed, its `roofline` block (per-launch fraction, traffic, VALU issue) whole."""
    import subprocess
    warm, steps = EXTRA_WINDOWS.get(name, (10, 100))
    if args.extra_steps > 0:
        steps = args.extra_steps
    cmd = [sys.executable, os.path.abspath(__file__), "--config", name, "--gpus", "1", "--steps", str(steps), "--warmup", str(warm), "--no-cpu-baseline",
           "--no-second-window", "--no-extra-configs", "--pgs-schedule", str(pgs), "--timing-stride", str(args.timing_stride)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK", "ROLE_RANK", "TORCHELASTIC_RUN_ID")}
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    wall = time.perf_counter() - t0
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    if r.returncode != 0 or not lines:
        raise RuntimeError(f"bench.py --config {name}: rc {r.returncode}: {r.stderr[-800:]}")
    j = json.loads(lines[-1]); c = j["config"]; rf = j["roofline"]
    keep = {k: c[k] for k in c if k in ("ncon_histogram", "nefc_histogram", "objects_alive_per_env", "service_ms_per_churn", "churns", "max_ncon", "max_nefc",
                                         "contact_capacity", "launches_per_cohort_step", "pgs_order", "pgs_schedule", "timed_window_ms")}
    return {"value": j["value"], "unit": j["unit"], "envs": c["envs_per_gpu"], "steps": j["steps"], "warmup": j["warmup"], "settle_steps": c["settle_steps"],
            "ms_per_step": j["ms_per_step"], "with_inverse": c["with_inverse"], "cohorts": c["cohorts"], "envs_per_wavefront": c["envs_per_wavefront"],
            "steps_per_launch": c["steps_per_launch"], "kernel_ms": rf["kernel_ms"], "roofline_frac": rf["frac"], "roofline_achieved_GBs": rf["achieved"],
            "algorithmic_bytes_per_env_step": rf["algorithmic_bytes_per_env_step"], "mean_ncon": c["mean_ncon"], "mean_nefc": c["mean_nefc"],
            "mean_solver_iter": c["mean_solver_iter"], "overflow_envs": c["overflow_envs"], "workload": c["workload"], **keep,
            "roofline": rf, "process": "own (python bench.py --config %s --steps %d --warmup %d ...)" % (name, steps, warm), "process_wall_s": wall,
            **({"unsettled": True} if j.get("unsettled") else {})}


def extra_config_lines(args):
    """S24D, C2 - C5 and the metric's scene under the two other Gauss-Seidel schedules, one process each, BEFORE this process touches the GPU"""
    out = {}
    for name in ("s24d", "c2", "c3", "c4", "c5"):
        try:
            out[name] = child_config_line(args, name)
        except Exception as ex:   # an extra must never cost the headline
            out[name] = {"error": repr(ex)}
    # the metric's scene under the LEGACY patch order (mjh_set_pgs_row_order(0): contacts regrouped by body pair, first-fit steps — the
    # round-3 default) and with the row order walked strictly sequentially (2): what the reference's order costs, and what the list schedule buys
    if args.pgs_schedule == 1:
        for key, mode in (("s24_legacy_patch_order", 0), ("s24_row_order_sequential", 2)):
            try:
                out[key] = child_config_line(args, "s24", pgs=mode)
            except Exception as ex:
                out[key] = {"error": repr(ex)}
    return out


def literal_loop_line(w, steps):
    """The LITERAL loop body of the reference (mj_main.cpp:82-112) on the main workload's engine: per step mjh_step1 ->
    MjHWInterface::read of env 0 (mjh_inverse + joint state to the host: a host synchronisation) -> controller_manager ->
    MjHWInterface::write of env 0 (command from the host) -> mjh_step2.  Two launches per cohort and two small transfers per step;
    only env 0's cohort waits for the host (include/mjhip.h, launch scheduling): what a ROS node that keeps the per-step hand-off
    gets; the fused mjh_step is what `value` measures."""
    e = w.eng
    cmd = np.zeros((1, e.nv))

    def literal(n):
        for _ in range(n):
            e.step1(); e.inverse()               # (one launch: mjh_step1 defers to the next entry point, include/mjhip.h)
            e.get_joint_state(0, 1)
            e.set_cmd(ddq=cmd, dq=None, env0=0)
            e.step2()

    def fused(n):
        for _ in range(n):
            e.step(1, True)
            e.get_joint_state(0, 1)
            e.set_cmd(ddq=cmd, dq=None, env0=0)

    # This loop waits for the device once per step, so a pause of the HOST lands in the result whole: with torch imported a full
    # pass of CPython's cycle collector takes 35-60 ms — as long as the timed window itself — and fell into the window of about
    # every second run (tools/literal_bench_probe.py: median wait 0.36 ms, one wait of 36-59 ms).  The collector is run before and
    # held off during the two windows, as around any latency measurement; a C++ host (the reference's loop) has none.
    import gc
    literal(5); e.synchronize()                  # (first use of the split entry points: launch-order buffer, full-range sort)
    gc.collect(); gc_was = gc.isenabled(); gc.disable()
    try:
        t0 = time.perf_counter(); literal(steps); e.synchronize(); dt = time.perf_counter() - t0
        fused(5); e.synchronize()
        t0 = time.perf_counter(); fused(steps); e.synchronize(); dt2 = time.perf_counter() - t0
    finally:
        if gc_was: gc.enable()
    return {"value": w.nenv * steps / dt, "unit": "env-steps/s", "ms_per_step": dt / steps * 1e3, "steps": steps, "envs": w.nenv,
            "sequence": "mjh_step1 -> mjh_inverse + mjh_get_joint_state(env 0) -> mjh_set_cmd(env 0) -> mjh_step2 (2 launches — step1 + inverse fused —, 2 host transfers per step)",
            "fused_step_with_per_step_read_write": {"value": w.nenv * steps / dt2, "ms_per_step": dt2 / steps * 1e3}}


DUMP_BUDGET_BYTES = 64 << 20


def dump_outputs(w, out_dir, rank=0, world=1):
    """The state the timed path leaves after its last step, per environment, as <out_dir>/<name>.npy (float64; the device's fp32
    values convert exactly): time, qpos, qvel, qacc_warmstart (mjh_get_state) and stats = ncon, nefc, solver sweeps, flags of the
    environment's wavefront (mjh_get_stats).  env_ids holds the global ids of the rows written: every environment, or a fixed,
    seeded sample of them where the whole set would exceed 64 MB.  N > 1: one set per rank, the names suffixed _rank<r>."""
    n = w.nenv
    q, v, ws, _ = w.env_state(n)
    t = w.eng.get_state(0, w.rows)[0]
    st = w.eng.get_stats(0, w.rows)
    save_outputs(out_dir, {"time": np.repeat(t, w.pack)[:n], "qpos": q, "qvel": v, "qacc_warmstart": ws,
                           "stats": np.repeat(st.astype(np.float64), w.pack, axis=0)[:n],
                           "env_ids": np.arange(w.env_offset, w.env_offset + n, dtype=np.float64)}, f"_rank{rank}" if world > 1 else "")


def save_outputs(out_dir, arrs, sfx=""):
    """arrays of one row per environment -> <out_dir>/<name><sfx>.npy in float64, a seeded sample of the rows above the 64 MB budget"""
    n = len(arrs["env_ids"])
    total = sum(a.size * 8 for a in arrs.values())
    if total > DUMP_BUDGET_BYTES:
        keep = np.sort(np.random.default_rng(0x0D0).choice(n, max(1, n * DUMP_BUDGET_BYTES // total), replace=False))
        arrs = {k: a[keep] for k, a in arrs.items()}
    os.makedirs(out_dir, exist_ok=True)
    for k, a in arrs.items():
        np.save(os.path.join(out_dir, f"{k}{sfx}.npy"), np.ascontiguousarray(a, dtype=np.float64))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--config", choices=sorted(WORKLOADS), default="s24", help="BASELINE.json config (default: the metric's scene, S24)")
    ap.add_argument("--envs-per-gpu", type=int, default=0, help="0 = the config's size (S24/C2/C5 4096, C3 8192, C4 2048)")
    ap.add_argument("--with-inverse", type=int, default=-1, help="mj_inverse every step in the MAIN timed window (-1: the config's default; the other variant is timed in a second window)")
    ap.add_argument("--cohorts", type=int, default=-1, help="env cohorts stepped on separate HIP streams (-1: the config's default, else the engine's)")
    ap.add_argument("--steps-per-launch", type=int, default=0, help="cap of the in-kernel step loop (0: the engine's default, 8; 1: one launch per step)")
    ap.add_argument("--timing-stride", type=int, default=5, help="bracket every N-th step launch with HIP events (roofline.kernel_ms is their mean)")
    ap.add_argument("--pack", type=int, default=0, help="environments per wavefront for the small-model configs (0: the config's default — C3 4, C5 2, others 1)")
    ap.add_argument("--pen-half", type=float, default=0.0, help="s24d: half width of the pen in metres (default 0.175, S24's own pen)")
    ap.add_argument("--maxcon", type=int, default=0, help="override the scene's contact capacity per env; 0 = scene default")
    ap.add_argument("--pgs-schedule", type=int, default=1, choices=[0, 1, 2],
                    help="mjh_set_pgs_row_order: 1 (default) mj_solPGS's own row order, independent blocks side by side under a precedence-preserving list "
                         "schedule; 2 the same order strictly one block after the other (bit-identical results); 0 the legacy reordering schedules (patch / group first fit)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-gather", action="store_true")
    ap.add_argument("--no-second-window", action="store_true", help="skip the second timed window (the other mj_inverse variant)")
    ap.add_argument("--force-dist", action="store_true", help="initialise torch.distributed and run the publish all-gather even with one rank (self-test of the multi-GPU path)")
    ap.add_argument("--host", choices=["ranks", "group"], default="ranks",
                    help="N > 1: `ranks` = one process per GPU over torch.distributed (what the driver launches; a plain invocation re-executes itself "
                         "under torch.distributed.run), `group` = ONE process driving every GPU through mjh_group_* (the C host API, RCCL all-gather)")
    ap.add_argument("--group-devices", default="", help="--host group: comma-separated device list (default 0..N-1; the same device twice is a one-GPU self-test on peer copies)")
    ap.add_argument("--no-extra-configs", action="store_true", help="--full, S24 at N = 1 appends short lines of the other BASELINE configs (c2..c5) and the literal loop; skip them")
    ap.add_argument("--extra-steps", type=int, default=0, help="timed steps of each appended config line (0: the config's own D3 window, EXTRA_WINDOWS — what the driver's line carries)")
    ap.add_argument("--rank-probe", action="store_true", help=argparse.SUPPRESS)     # tests: every rank prints its rank / world size and exits
    ap.add_argument("--full", action="store_true", help="also measure what takes runs of its own: second timed window, CPU baseline, "
                                                           "literal loop and the other configs (S24 at N = 1); off: the headline only")
    ap.add_argument("--dump-outputs", metavar="DIR", default="", help="write the state after the last timed step as DIR/<name>.npy (float64)")
    ap.add_argument("--cpu-envs", type=int, default=1024)
    ap.add_argument("--cpu-seconds", type=float, default=16.0, help="time budget of the CPU baseline sample")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.host == "group" and (args.gpus > 1 or args.group_devices):
        if "WORLD_SIZE" in os.environ and world > 1:
            raise SystemExit("--host group is ONE process for all GPUs: start it plainly, not under torch.distributed.run")
        return run_group_host(args)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        relaunch_under_torchrun(args)             # does not return
    if args.gpus > 1 and world != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} under a launcher with WORLD_SIZE={world}: start it with --nproc-per-node {args.gpus}, or plainly")
    if args.rank_probe:
        os.write(1, f"RANKPROBE {rank} {world} {local_rank}\n".encode())      # (one write: two ranks share the pipe)
        return

    # the other configs first, each in a process of its own, while this process has not created a stream yet (child_config_line)
    with_extras = args.full and rank == 0 and world == 1 and args.config == "s24" and not args.no_extra_configs and not args.force_dist
    extras_last = os.environ.get("BENCH_EXTRAS_LAST", "0") == "1"
    extras = extra_config_lines(args) if (with_extras and not extras_last) else None

    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1"); os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0"); os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    import mujoco_sim_amd as ms

    stream = torch.cuda.current_stream()
    from mujoco_sim_amd import capi
    capi.load().mjh_set_pgs_row_order(args.pgs_schedule)
    w = WORKLOADS[args.config](ms, args, rank, local_rank, stream.cuda_stream)
    eng, model, nenv = w.eng, w.model, w.nenv
    if args.cohorts > 0 or w.cohorts > 0:
        eng.set_cohorts(args.cohorts if args.cohorts > 0 else w.cohorts)
    if args.steps_per_launch > 0:
        eng.set_steps_per_launch(args.steps_per_launch)
    main_inverse = w.inverse if args.with_inverse < 0 else bool(args.with_inverse)
    stride = eng.state_stride
    pub = torch.empty(w.rows * stride, dtype=torch.float32, device="cuda")
    gathered = torch.empty(world * w.rows * stride, dtype=torch.float32, device="cuda") if use_dist else None
    publish_every = max(1, int(round(1.0 / (60.0 * model.opt.timestep))))  # 60 Hz of simulated time

    ag_events = []
    comm_stream = torch.cuda.Stream() if use_dist else None

    def run(nsteps, inverse, time_gather=False):
        left = nsteps
        while left > 0:
            k = left if args.no_gather else min(left, publish_every - w.step_count % publish_every)    # up to the next publish
            w.step(k, inverse); left -= k
            if not args.no_gather and w.step_count % publish_every == 0:   # 60 Hz publish: packed state slice (+ RCCL all-gather)
                if use_dist:
                    stream.wait_stream(comm_stream)        # the previous gather has read `pub` (three steps ago: long done)
                eng.export_state_device(pub.data_ptr())
                if use_dist:
                    # the collective runs on a stream of its own, beside the steps: on the stepping stream it would sit between two
                    # steps of every cohort (the next mjh_step forks from that stream) and drain the pipeline at every publish
                    comm_stream.wait_stream(stream)
                    with torch.cuda.stream(comm_stream):
                        if time_gather:
                            a_, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                            a_.record(); dist.all_gather_into_tensor(gathered, pub); b_.record(); ag_events.append((a_, b_))
                        else:
                            dist.all_gather_into_tensor(gathered, pub)

    def timed(nsteps, inverse):
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        # HIP events around step launches on the stream they are launched on (cohort streams); a sample of one launch in
        # `--timing-stride` so that the event pairs do not slow launch-bound configs down (C5: 34 M with every launch timed)
        eng.set_launch_timing(max(1, args.timing_stride))
        t0 = time.perf_counter()
        run(nsteps, inverse, time_gather=True)
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - t0
        if use_dist:
            tt = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        kernel_ms, n_timed = eng.get_launch_timing()
        eng.set_launch_timing(False)
        return elapsed, kernel_ms, n_timed

    # 1. the config's fixed settle phase — NOT --warmup: whatever the driver passes, the timed window steps the settled scene
    run(w.settle_steps, main_inverse)
    # 2. warm-up, 3. the timed window
    run(args.warmup, main_inverse)
    elapsed, kernel_ms, n_launches = timed(args.steps, main_inverse)
    st = eng.get_stats()
    total_envs = nenv * world
    value = total_envs * args.steps / elapsed
    cohorts = eng.cohorts
    bytes_step = algorithmic_bytes_per_env_step(w.base_model.nq, w.base_model.nv)
    G = cohorts if (cohorts > 1 and w.rows >= 64 * cohorts) else 1      # the engine's rule (engine.hip: mjh_step)
    envs_per_launch = nenv / G                                          # one launch = one step of one cohort
    n_timed, n_launches = n_launches, args.steps * G
    # steps one launch runs (in-kernel step loop: the stretch between two publishes, at most the engine's cap; 1: a launch per step)
    spl = int(eng.steps_per_launch) if args.no_gather else min(int(eng.steps_per_launch), publish_every)
    n_launches = -(-args.steps // spl) * G
    achieved = bytes_step * envs_per_launch * spl / (kernel_ms * 1e-3) / 1e9
    if args.dump_outputs:
        dump_outputs(w, args.dump_outputs, rank, world)

    # 4. (--full) the other mj_inverse variant, same K steps (the reference always pays mj_inverse,
    # mj_hw_interface.cpp:61 — report both)
    other = None
    if args.full and not args.no_second_window:
        e2, k2, n2 = timed(args.steps, not main_inverse)
        other = {"value": total_envs * args.steps / e2, "ms_per_step": e2 / args.steps * 1e3, "kernel_ms": k2}

    # committed rocprofv3 PMC measurement of this config (profiles/), per launch: provenance stated, never re-measured here
    traffic = traffic_src = valu_busy = valu_frac = valu_lanes = valu_instr = valu_fracs = None
    tpath = os.path.join(ROOT, "profiles", "hbm_traffic.json")
    if os.path.exists(tpath):
        try:
            tj = json.load(open(tpath))
            tj = tj.get(w.name, tj if (w.name == "s24" and "bytes_per_launch" in tj) else None)
            if tj and tj.get("bytes_per_launch") and tj.get("envs_per_launch"):
                traffic = tj["bytes_per_launch"] * envs_per_launch / tj["envs_per_launch"]
                valu_busy = tj.get("valu_issue_busy")
                valu_instr = tj.get("valu_instr_per_env_step"); valu_lanes = tj.get("valu_lane_util")
                if valu_instr:
                    # wave-instructions per second at THIS run's rate over the chip's 1024 SIMDs, against (i) the guide's issue peak — a
                    # wave64 fp32 VALU instruction every 2 clocks per SIMD (MI355X_MICROARCH.md) — which is `valu_issue_frac`, (ii) what this
                    # repo's micro-benchmark reaches with four resident waves per SIMD (one per 2.5 clocks: profiles/r02m_valu_issue_bench.txt)
                    # and (iii) the rate of a LONE wave (one per 8 clocks) — the window kernel's 424 registers leave one wave per SIMD, so (iii)
                    # is the ceiling of the structure and the number that says how full the SIMDs' only wave keeps its own issue slots
                    vrate = valu_instr * (value / world) / 1024 / 2.4e9          # VALU instructions per SIMD and clock
                    valu_frac = vrate * 2.0
                    valu_fracs = {"per_2_clocks_guide_peak": vrate * 2.0, "per_2.5_clocks_measured_4_waves": vrate * 2.5, "per_8_clocks_lone_wave": vrate * 8.0}
                traffic_src = f"profiles/{tj.get('tag', '?')} (committed rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this config, scaled to this run's envs per launch; not measured in this run)"
        except Exception:
            traffic = None
    mean_ncon = float(st[:, 0].mean()) / w.pack
    unsettled = w.min_ncon is not None and mean_ncon < w.min_ncon
    key_inv, key_no = ("value", "value_without_inverse") if main_inverse else ("value_with_inverse", "value")
    out = {
        "metric": METRIC if w.name == "s24" else f"env-steps/sec (whole node), BASELINE config {w.name.upper()}",
        "value": value, "unit": "env-steps/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f32", "data": "synthetic",
        "config": {"workload": w.label, "name": w.name, "settle_steps": w.settle_steps, "envs_per_gpu": nenv, "envs_total": total_envs,
                   "steps_per_launch": spl, "launches_per_cohort_step": int(eng.launches_per_step), "cohorts": cohorts, "with_inverse": bool(main_inverse), "parallelism": f"env-sharded x{world}",
                   "envs_per_wavefront": w.pack, "nq": int(w.base_model.nq), "nv": int(w.base_model.nv),
                   "mean_ncon": mean_ncon, "max_ncon": int(st[:, 0].max()), "mean_nefc": float(st[:, 1].mean()) / w.pack,
                   "max_nefc": int(st[:, 1].max()), "mean_solver_iter": float(st[:, 2].mean()),
                   "overflow_envs": int((st[:, 3] & 3 != 0).sum()), "reset_envs": int((st[:, 3] & 4 != 0).sum()),
                   "lds_bytes_per_env": eng.lds_bytes, "contact_capacity": int(model.maxcon),
                   "pgs_order": ["legacy: independent pairs / groups of blocks (first fit)", "legacy: contact patches sorted by body pair (first fit)", "mj_solPGS row order"][eng.solver_order()],
                   "pgs_schedule": ["legacy reordering schedule", "precedence-preserving list schedule (bit-identical to the sequential sweep)", "sequential, one block after the other"][eng.pgs_schedule()],
                   "solver_form": ("window sweep: assemble launch + mjh_window_kernel (16 consecutive rows per window, four envs per wavefront; 64-row windows, one env per wavefront, for the envs with the most rows)" if eng.window_solver()
                                   else "dense row-space sweeps (AR on the matrix cores) for cohorts with a long-sweeping env, constraint blocks elsewhere" if eng.dense_solver()
                                   else "contact patches (<= 16 rows of one body pair, <= 4 side by side)" if eng.patch_sweep() else "constraint blocks"),
                   "timed_window_ms": elapsed * 1e3, **w.extra_config()},
        "roofline": {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
                     "traffic": traffic, "traffic_source": traffic_src,
                     "kernel": ("mjh_step_kernel (assemble: position / velocity stages, collision, constraint rows) + mjh_window_kernel (PGS sweeps in mj_solPGS row order, four "
                                "envs per wavefront in 16-row windows, one env per wavefront in 64-row windows above 96 rows (S24) / above 192 rows (models whose rows can exceed 256: S24D) —, rows in registers; mj_Euler): the two-launch chain of one cohort's step, timed as one" if eng.window_solver() else "mjh_step_kernel") + ((" (+ mjh_dense_build_kernel [MFMA] + mjh_dense_solve_kernel: assemble -> build -> solve -> integrate chain of the many-body layout)" if eng.dense_solver() else
                                                     " (+ mjh_solve_kernel: three-launch step of the many-body layout)") if eng.lds_bytes > 24 * 1024 or model.nv > 64 else ""),
                     "kernel_ms": kernel_ms, "launches": n_launches, "launches_timed": n_timed, "envs_per_launch": envs_per_launch, "concurrent_launches": cohorts,
                     # `achieved` / `frac` are per launch (one cohort's step), as the contract defines them; the cohorts' launches overlap, so the
                     # chip as a whole moves the algorithmic bytes of ALL envs per step period:
                     "achieved_whole_chip": bytes_step * nenv / (elapsed / args.steps) / 1e9, "frac_whole_chip": bytes_step * nenv / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                     "algorithmic_bytes_per_env_step": bytes_step,
                     # the second fraction (say which binds): VALU issue — committed SQ-counter passes of this config x this run's rate
                     "valu_issue_frac": valu_frac, "valu_issue_frac_by_denominator": valu_fracs, "valu_lane_util": valu_lanes, "valu_instr_per_env_step": valu_instr,
                     "valu_source": traffic_src.replace("FETCH_SIZE / WRITE_SIZE", "SQ_INSTS_VALU / SQ_ACTIVE_INST_VALU / SQ_THREAD_CYCLES_VALU") if (traffic_src and valu_instr) else None,
                     "binds": ((("the dependent instruction chain of ONE resident wave per SIMD (window kernel: 424 registers): " if w.name in ("s24", "s24d") else
                                 "the dependent instruction chain of the one wavefront an environment (or a pack of them) is stepped by, few of them per SIMD: ") +
                                "a lone wave issues at most one VALU instruction per 8 clocks — valu_issue_frac_by_denominator.per_8_clocks_lone_wave says how much of THAT the chip uses; "
                                "against the SIMD's issue peak it is valu_issue_frac; HBM (frac) does not bind")) if valu_frac else None,
                     "timed_window_note": f"{args.steps} steps = {elapsed * 1e3:.1f} ms; kernel_ms is the mean of {n_timed} event-timed launches in it",
                     "note": "fused per-env pipeline keeps intermediates in LDS / registers: the path is issue/latency bound, far below the HBM roofline by design (DESIGN.md §4, §5)"},
    }
    if other is not None:
        out[key_inv if not main_inverse else key_no] = other["value"]
        out["second_window"] = {"with_inverse": not main_inverse, **other}
    if unsettled:
        out["unsettled"] = True; out["valid"] = False
        out["note"] = f"mean_ncon {mean_ncon:.1f} < {w.min_ncon}: the scene is not in the state the metric names — do not use `value`"
    if use_dist:
        from mujoco_sim_amd import shard
        ag_ms = [a_.elapsed_time(b_) for a_, b_ in ag_events]
        out["host"] = {"kind": "ranks", "api": "one process per GPU under torch.distributed.run; dist.all_gather_into_tensor over RCCL", "rccl_ranks": world,
                       "ranks": [{"rank": r, "env0": shard.env_range(total_envs, world, r)[0], "nenv": shard.env_range(total_envs, world, r)[1] - shard.env_range(total_envs, world, r)[0]} for r in range(world)],
                       "all_gather": {"ms_mean": float(np.mean(ag_ms)) if ag_ms else None, "count": len(ag_ms), "bytes_per_rank": int(w.rows * stride * 4),
                                      "publish_every_steps": publish_every, "note": "stream time of the collective on rank 0 (includes waiting for the slowest rank's pack)"}}
    if with_extras:
        # the literal reference loop on this engine, in the SAME line (extra key)
        try:
            out["literal_loop"] = literal_loop_line(w, max(50, min(args.steps, 200)))
        except Exception as ex:   # an extra must never cost the headline
            out["literal_loop"] = {"error": repr(ex)}
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:   # the CPU baseline is timed at N = 1 only
        out["cpu_baseline"] = cpu_baseline(w, args.cpu_envs, args.cpu_seconds, main_inverse)
    if use_dist:
        dist.barrier()
    eng.close()
    if with_extras and extras_last:
        extras = extra_config_lines(args)
    if extras is not None:
        out["configs"] = extras
        d = extras.get("s24d", {})
        if "value" in d:
            # the "30-contact" reading of the metric's name, where the driver's parser sees it: S24 (D2-exact, `value`) settles at ~17 contacts /
            # ~75 rows, S24D (same boxes released 2 x 2) at ~32 / ~138 ("print the measured ncon so the ~30 claim is checked")
            out["value_30_contact"] = d["value"]
            out["roofline_30_contact"] = d["roofline"]
            out["config_30_contact"] = {k: d.get(k) for k in ("workload", "envs", "steps", "warmup", "settle_steps", "ms_per_step", "cohorts", "mean_ncon", "max_ncon", "mean_nefc",
                                                                "max_nefc", "mean_solver_iter", "overflow_envs", "contact_capacity", "ncon_histogram", "nefc_histogram")}
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        try:  # RCCL prints its banner through C stdio: flush it first so that the JSON is the LAST line of stdout
            import ctypes
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
