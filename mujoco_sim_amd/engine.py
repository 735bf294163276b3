"""Thin Python mirror of the C ABI: a `Model` (compiled scene) and an `Engine`
(nenv environments on one HIP device).  Names follow the reference's step loop
(src/mj_main.cpp:76-113): step1 / inverse / step2 / forward, set_cmd == MjHWInterface::write,
get_joint_state == MjHWInterface::read.  All compute happens in libmjhip.so."""
import ctypes as C

import numpy as np

from . import capi


class MjhError(RuntimeError):
    pass


def _chk(lib, rc, what):
    if rc is not None and rc < 0:
        raise MjhError(f"{what} failed ({rc}): {lib.mjh_last_error().decode()}")
    return rc


class Model:
    """Owns an mjh_model*."""

    def __init__(self, ptr, lib=None):
        self.lib = lib or capi.load()
        if not ptr:
            raise MjhError("model build failed: " + self.lib.mjh_last_error().decode())
        self.ptr = ptr
        self.c = ptr.contents

    def __getattr__(self, name):
        c = self.__dict__.get("c")
        if c is not None and name in capi._INT_SIZES + capi._INT_SIZES2 + capi._INT_SIZES4 + capi._INT_SIZES6 + capi._INT_SIZES7 + capi._INT_SIZES9 + capi._INT_SIZES10 + ["meaninertia", "opt"]:
            return getattr(c, name)
        raise AttributeError(name)

    def array(self, name):
        return self.c.array(name)

    def name2id(self, objtype, name):
        return self.lib.mjh_name2id(self.ptr, objtype, name.encode())

    def ray_skipped_geoms(self):
        """geoms no ray can see in mesh mode 0: mesh geoms and hfield geoms without an asset (mjh_ray_skipped_geoms)"""
        return self.lib.mjh_ray_skipped_geoms(self.ptr)

    def replicate(self, copies):
        """sub-wave packing: `copies` instances of the moving bodies in one model (mjh_model_replicate)"""
        return Model(self.lib.mjh_model_replicate(self.ptr, int(copies)), self.lib)

    def s24_randomize(self, env0, nenv, seed_base=0x5EED0000):
        """Per-env S24 tables: dict of float64 arrays."""
        c = self.c
        out = dict(
            qpos=np.zeros((nenv, c.nq)), geom_size=np.zeros((nenv, 3 * c.ngeom)), geom_rbound=np.zeros((nenv, c.ngeom)),
            body_mass=np.zeros((nenv, c.nbody)), body_inertia=np.zeros((nenv, 3 * c.nbody)),
            body_invweight0=np.zeros((nenv, 2 * c.nbody)), dof_invweight0=np.zeros((nenv, c.nv)))
        rc = self.lib.mjh_scene_s24_randomize(self.ptr, env0, nenv, seed_base, *[capi.dptr(out[k]) for k in
                                              ["qpos", "geom_size", "geom_rbound", "body_mass", "body_inertia",
                                               "body_invweight0", "dof_invweight0"]])
        _chk(self.lib, rc, "mjh_scene_s24_randomize")
        return out


def boxes_randomize(model, env0, nenv, seed_base=0x5EED0000, jitter=0.01):
    """Per-env tables of a free-box scene (C2): dict of float64 arrays like Model.s24_randomize."""
    c = model.c
    out = dict(
        qpos=np.zeros((nenv, c.nq)), geom_size=np.zeros((nenv, 3 * c.ngeom)), geom_rbound=np.zeros((nenv, c.ngeom)),
        body_mass=np.zeros((nenv, c.nbody)), body_inertia=np.zeros((nenv, 3 * c.nbody)),
        body_invweight0=np.zeros((nenv, 2 * c.nbody)), dof_invweight0=np.zeros((nenv, c.nv)))
    rc = model.lib.mjh_scene_boxes_randomize(model.ptr, env0, nenv, seed_base, float(jitter), *[capi.dptr(out[k]) for k in
                                             ["qpos", "geom_size", "geom_rbound", "body_mass", "body_inertia",
                                              "body_invweight0", "dof_invweight0"]])
    _chk(model.lib, rc, "mjh_scene_boxes_randomize")
    return out


def load_mjcf(xml=None, path=None, paths=None, textures=False):
    """MJCF-subset loader (mj_loadXML boundary, mj_util.h:185-193); `paths`: world file + robot files composed into one model;
    `textures`: load builtin 2D textures for this call (mjh_load_set_textures 1; the thread's setting is 0 again afterwards)"""
    lib = capi.load()
    if textures:
        lib.mjh_load_set_textures(1)
    try:
        if paths:
            arr = (C.c_char_p * len(paths))(*[p.encode() for p in paths])
            ptr = lib.mjh_load_mjcf_files(arr, len(paths))
        else:
            ptr = lib.mjh_load_mjcf_file(path.encode()) if path else lib.mjh_load_mjcf_string(xml.encode())
    finally:
        if textures:
            lib.mjh_load_set_textures(0)
    m = Model(ptr, lib)
    m.note = lib.mjh_load_note().decode()
    return m


def scene(name, *args):
    lib = capi.load()
    fn = {"s24": lib.mjh_scene_s24, "s24pen": lib.mjh_scene_s24_pen, "pendulum": lib.mjh_scene_pendulum, "arm7": lib.mjh_scene_arm7,
          "boxpile": lib.mjh_scene_boxpile}[name]
    return Model(fn(*args), lib)


def set_contact_report(on):
    """mjh_set_contact_report: engines created afterwards (process-wide); Engine(..., contact_report=True) sets it for one engine"""
    capi.load().mjh_set_contact_report(1 if on else 0)


EP = dict(geom_size=0, geom_rbound=1, body_mass=2, body_inertia=3, body_invweight0=4, dof_invweight0=5)


def device_buffer(buf, name, count, device=0, dtypes=("float32",)):
    """Address of a device buffer argument of the *_device calls.  None -> None and an integer address is taken as is.  An object with
    data_ptr() (a torch tensor) must have one of `dtypes`, be contiguous, hold exactly `count` elements and live on CUDA/HIP device
    `device`; each failure raises MjhError naming the argument.  This check is what keeps a host tensor's address from reaching a kernel."""
    if buf is None:
        return None
    if isinstance(buf, (int, np.integer)):
        return int(buf)
    if not hasattr(buf, "data_ptr"):
        raise MjhError(f"{name}: expected a device address or an object with data_ptr(), got {type(buf).__name__}")
    dtype = str(buf.dtype).split(".")[-1]
    if dtype not in dtypes:
        raise MjhError(f"{name}: dtype {dtype}, expected {' or '.join(dtypes)}")
    if not buf.is_contiguous():
        raise MjhError(f"{name}: not contiguous")
    if int(buf.numel()) != int(count):
        raise MjhError(f"{name}: {int(buf.numel())} elements, expected {int(count)}")
    dev = buf.device
    if dev.type != "cuda" or (dev.index if dev.index is not None else 0) != device:
        raise MjhError(f"{name}: on device {dev}, expected cuda:{device} (the engine's)")
    return int(buf.data_ptr())


def _buffer_rows(buf, width):
    """rows of a buffer argument of width `width`, or None for an address / None"""
    if buf is None or not hasattr(buf, "data_ptr"):
        return None
    return int(buf.shape[0]) if buf.dim() >= 2 else int(buf.numel()) // max(width, 1)


class Engine:
    def __init__(self, model, nenv, device=0, stream=None, contact_report=False):
        """contact_report: the engine leaves the contacts with their solver forces and cfrc_ext on the device after every solve
        (mjh_set_contact_report around mjh_create; the process-wide switch is put back afterwards).  False leaves the switch as it is:
        set_contact_report() or MJH_CONTACT_REPORT then decide, and `contact_report` tells what the engine does"""
        self.lib = model.lib
        self.model = model
        self.nenv = nenv
        self.device = device
        h = C.c_void_p()
        if contact_report:
            probe_was = self.lib.mjh_contact_report(None)      # (no engine: the process-wide switch)
            self.lib.mjh_set_contact_report(1)
            try:
                rc = self.lib.mjh_create(model.ptr, nenv, device, C.c_void_p(stream or 0), C.byref(h))
            finally:
                self.lib.mjh_set_contact_report(probe_was)
            _chk(self.lib, rc, "mjh_create")
        else:
            _chk(self.lib, self.lib.mjh_create(model.ptr, nenv, device, C.c_void_p(stream or 0), C.byref(h)), "mjh_create")
        self.h = h
        self.nq, self.nv, self.nbody, self.ngeom = model.nq, model.nv, model.nbody, model.ngeom

    @classmethod
    def from_handle(cls, model, handle, nenv, device=0):
        """view of an engine owned by someone else (a device of an mjh_group): close() does not destroy it"""
        self = cls.__new__(cls)
        self.lib = model.lib; self.model = model; self.nenv = nenv; self.h = C.c_void_p(handle); self._borrowed = True; self.device = device
        self.nq, self.nv, self.nbody, self.ngeom = model.nq, model.nv, model.nbody, model.ngeom
        return self

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.lib.mjh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- stepping (mj_main.cpp:83-110)
    def step1(self): _chk(self.lib, self.lib.mjh_step1(self.h), "mjh_step1")
    def step2(self): _chk(self.lib, self.lib.mjh_step2(self.h), "mjh_step2")
    def inverse(self): _chk(self.lib, self.lib.mjh_inverse(self.h), "mjh_inverse")
    def forward(self): _chk(self.lib, self.lib.mjh_forward(self.h), "mjh_forward")
    def step(self, n=1, with_inverse=False): _chk(self.lib, self.lib.mjh_step(self.h, n, int(with_inverse)), "mjh_step")
    def synchronize(self): _chk(self.lib, self.lib.mjh_synchronize(self.h), "mjh_synchronize")

    def set_timestep(self, dt): _chk(self.lib, self.lib.mjh_set_timestep(self.h, float(dt)), "mjh_set_timestep")
    @property
    def timestep(self): return self.lib.mjh_get_timestep(self.h)

    # ---- launch scheduling / timing (include/mjhip.h "launch scheduling")
    def set_cohorts(self, n): _chk(self.lib, self.lib.mjh_set_cohorts(self.h, int(n)), "mjh_set_cohorts")
    @property
    def cohorts(self): return self.lib.mjh_get_cohorts(self.h)
    def set_steps_per_launch(self, n): _chk(self.lib, self.lib.mjh_set_steps_per_launch(self.h, int(n)), "mjh_set_steps_per_launch")
    @property
    def steps_per_launch(self): return self.lib.mjh_get_steps_per_launch(self.h)
    @property
    def launches_per_step(self):
        """host-side launches mjh_step issues per cohort-step (1: fused kernel, or a launch chain queued as one captured graph)"""
        return self.lib.mjh_launches_per_step(self.h)

    def set_launch_timing(self, on=True): _chk(self.lib, self.lib.mjh_set_launch_timing(self.h, int(on)), "mjh_set_launch_timing")   # N > 1: every N-th launch
    def get_launch_timing(self):
        """-> (mean step-kernel duration [ms], launches) since the last call"""
        ms_, cnt = C.c_double(0), C.c_int(0)
        _chk(self.lib, self.lib.mjh_get_launch_timing(self.h, C.byref(ms_), C.byref(cnt)), "mjh_get_launch_timing")
        return ms_.value, cnt.value

    # ---- commands (mj_hw_interface.cpp:73-91)
    def set_cmd(self, ddq=None, dq=None, env0=0):
        a = None if ddq is None else np.ascontiguousarray(ddq, dtype=np.float64).reshape(-1, self.nv)
        b = None if dq is None else np.ascontiguousarray(dq, dtype=np.float64).reshape(-1, self.nv)
        n = (a if a is not None else b).shape[0]
        _chk(self.lib, self.lib.mjh_set_cmd(self.h, env0, n, capi.dptr(a), capi.dptr(b)), "mjh_set_cmd")

    def set_pd_controller(self, kp, kd):
        """in-engine joint-space PD effort controller (ros_control's effort controllers for all envs at once)"""
        _chk(self.lib, self.lib.mjh_set_pd_controller(self.h, float(kp), float(kd)), "mjh_set_pd_controller")

    def set_pd_target(self, target, env0=0):
        t = np.ascontiguousarray(target, dtype=np.float64).reshape(-1, self.nv)
        _chk(self.lib, self.lib.mjh_set_pd_target(self.h, env0, t.shape[0], capi.dptr(t)), "mjh_set_pd_target")

    def set_controlled_dofs(self, mask):
        m = np.ascontiguousarray(mask, dtype=np.int32)
        _chk(self.lib, self.lib.mjh_set_controlled_dofs(self.h, capi.iptr(m)), "mjh_set_controlled_dofs")

    def set_odom(self, lin, ang, angq):
        a, b, c = (np.ascontiguousarray(x, dtype=np.int32) for x in (lin, ang, angq))
        _chk(self.lib, self.lib.mjh_set_odom_dofs(self.h, capi.iptr(a), capi.iptr(b), capi.iptr(c)), "mjh_set_odom_dofs")

    def set_odom_vel(self, twist, env0=0):
        t = np.ascontiguousarray(twist, dtype=np.float64).reshape(-1, 6)
        _chk(self.lib, self.lib.mjh_set_odom_vel(self.h, env0, t.shape[0], capi.dptr(t)), "mjh_set_odom_vel")

    # ---- state
    def get_state(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        t = np.zeros(n); q = np.zeros((n, self.nq)); v = np.zeros((n, self.nv)); w = np.zeros((n, self.nv))
        _chk(self.lib, self.lib.mjh_get_state(self.h, env0, n, capi.dptr(t), capi.dptr(q), capi.dptr(v), capi.dptr(w)), "mjh_get_state")
        return t, q, v, w

    def set_state(self, qpos=None, qvel=None, time=None, warmstart=None, env0=0):
        arrs = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (time, qpos, qvel, warmstart)]
        n = next(a for a in arrs if a is not None)
        n = n.shape[0] if n.ndim > 1 or arrs[0] is n else 1
        if qpos is not None:
            n = arrs[1].reshape(-1, self.nq).shape[0]
        elif qvel is not None:
            n = arrs[2].reshape(-1, self.nv).shape[0]
        _chk(self.lib, self.lib.mjh_set_state(self.h, env0, n, *[capi.dptr(a) for a in arrs]), "mjh_set_state")

    def get_joint_state(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        q = np.zeros((n, self.nq)); v = np.zeros((n, self.nv)); f = np.zeros((n, self.nv))
        _chk(self.lib, self.lib.mjh_get_joint_state(self.h, env0, n, capi.dptr(q), capi.dptr(v), capi.dptr(f)), "mjh_get_joint_state")
        return q, v, f

    def get_body_state(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        p = np.zeros((n, self.nbody, 3)); q = np.zeros((n, self.nbody, 4))
        _chk(self.lib, self.lib.mjh_get_body_state(self.h, env0, n, capi.dptr(p), capi.dptr(q)), "mjh_get_body_state")
        return p, q

    def get_geom_state(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        p = np.zeros((n, self.ngeom, 3)); m = np.zeros((n, self.ngeom, 9))
        _chk(self.lib, self.lib.mjh_get_geom_state(self.h, env0, n, capi.dptr(p), capi.dptr(m)), "mjh_get_geom_state")
        return p, m

    def get_field(self, name, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        w = 2 if name == "energy" else self.nv
        out = np.zeros((n, w))
        _chk(self.lib, self.lib.mjh_get_field(self.h, name.encode(), env0, n, capi.dptr(out)), "mjh_get_field")
        return out

    def get_stats(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        out = np.zeros((n, 4), dtype=np.int32)
        _chk(self.lib, self.lib.mjh_get_stats(self.h, env0, n, capi.iptr(out)), "mjh_get_stats")
        return out

    def get_contacts(self, env):
        mc = self.model.maxcon
        dist = np.zeros(mc); pos = np.zeros((mc, 3)); fr = np.zeros((mc, 9)); g = np.zeros((mc, 2), dtype=np.int32)
        n = _chk(self.lib, self.lib.mjh_get_contacts(self.h, env, capi.dptr(dist), capi.dptr(pos), capi.dptr(fr), capi.iptr(g)), "mjh_get_contacts")
        return dict(dist=dist[:n], pos=pos[:n], frame=fr[:n], geom=g[:n])

    # ---- contact report (Engine(..., contact_report=True)): contacts with their solver forces, cfrc_ext, per-body contact force
    @property
    def contact_report(self):
        """True when this engine leaves the contact report after every solve (mjh_contact_report)"""
        return bool(self.lib.mjh_contact_report(self.h))

    def contact_forces(self, env0=0, n=None):
        """the report of the last solve: dict of ncon [n] and, per env, lists trimmed to its ncon: dist [k], pos [k, 3], frame [k, 9], force
        [k, 6] (mj_contactForce's layout, contact frame, on geom2's body; entries 4 and 5 are zero), geom [k, 2], dim [k]"""
        n = self.nenv - env0 if n is None else n
        mc = self.model.maxcon
        ncon = np.zeros(n, dtype=np.int32); dist = np.zeros((n, mc)); pos = np.zeros((n, mc, 3)); fr = np.zeros((n, mc, 9))
        force = np.zeros((n, mc, 6)); geom = np.zeros((n, mc, 2), dtype=np.int32); dim = np.zeros((n, mc), dtype=np.int32)
        _chk(self.lib, self.lib.mjh_get_contact_forces(self.h, env0, n, capi.iptr(ncon), capi.dptr(dist), capi.dptr(pos), capi.dptr(fr),
                                                       capi.dptr(force), capi.iptr(geom), capi.iptr(dim)), "mjh_get_contact_forces")
        trim = lambda a: [a[i, :ncon[i]].copy() for i in range(n)]
        return dict(ncon=ncon, dist=trim(dist), pos=trim(pos), frame=trim(fr), force=trim(force), geom=trim(geom), dim=trim(dim))

    def cfrc_ext(self, env0=0, n=None):
        """d->cfrc_ext of the last solve [n, nbody, 6]: torque(3) force(3), world axes, about the subtree COM of the body's tree root"""
        n = self.nenv - env0 if n is None else n
        out = np.zeros((n, self.nbody, 6))
        _chk(self.lib, self.lib.mjh_get_cfrc_ext(self.h, env0, n, capi.dptr(out)), "mjh_get_cfrc_ext")
        return out

    @staticmethod
    def _selection(bodies, against):
        b = np.ascontiguousarray(np.atleast_1d(bodies), dtype=np.int32)
        a = None if against is None else np.ascontiguousarray(np.broadcast_to(np.atleast_1d(against), b.shape), dtype=np.int32)
        return b, a

    def body_contact_force(self, bodies, against=None, env0=0, n=None):
        """net contact force ON each of `bodies` in world axes [n, nsel, 3] and the number of contacts in each sum [n, nsel];
        against: per body the other body a contact must touch to count (-1 / None: any)"""
        n = self.nenv - env0 if n is None else n
        b, a = self._selection(bodies, against)
        force = np.zeros((n, len(b), 3)); count = np.zeros((n, len(b)), dtype=np.int32)
        _chk(self.lib, self.lib.mjh_body_contact_force(self.h, env0, n, len(b), capi.iptr(b), capi.iptr(a), capi.dptr(force), capi.iptr(count)),
             "mjh_body_contact_force")
        return force, count

    def body_contact_force_device(self, d_force, d_count, bodies, against=None, env0=0, n=None):
        """mjh_body_contact_force_device: device addresses (data_ptr()) of fp32 force [n, nsel, 3] and int32 count [n, nsel] (d_count may be
        None); enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        b, a = self._selection(bodies, against)
        _chk(self.lib, self.lib.mjh_body_contact_force_device(self.h, env0, n, len(b), capi.iptr(b), capi.iptr(a), C.c_void_p(d_force), C.c_void_p(d_count)),
             "mjh_body_contact_force_device")

    def contact_report_device(self):
        """device addresses of the engine's report buffers: dict of ncon (int32 [nenv]), records (fp32 [nenv, maxcon, 20]), cfrc_ext
        (fp32 [nenv, nbody, 6]) and maxcon; they belong to the engine and hold the last solve's report once its stream has reached it"""
        p = [C.c_void_p(), C.c_void_p(), C.c_void_p()]; mc = C.c_int(0)
        _chk(self.lib, self.lib.mjh_contact_report_device(self.h, C.byref(p[0]), C.byref(p[1]), C.byref(p[2]), C.byref(mc)), "mjh_contact_report_device")
        return dict(ncon=p[0].value, records=p[1].value, cfrc_ext=p[2].value, maxcon=mc.value)

    # ---- frame states: pose, twist and Jacobian of bodies and sites (mjh_frame_state)
    _FRAME_TYPES = {"body": (0, 0), "site": (1, 3)}      # name -> (MJH_FRAME_*, objtype of mjh_name2id)

    def _frame_id(self, item, what):
        kind, ref = item
        if kind not in self._FRAME_TYPES:
            raise MjhError(f"{what}: frame type {kind!r} is neither 'body' nor 'site'")
        code, objtype = self._FRAME_TYPES[kind]
        if isinstance(ref, str):
            i = self.model.name2id(objtype, ref)
            if i < 0:
                raise MjhError(f"{what}: no {kind} named {ref!r}")
            return code, i
        return code, int(ref)

    def _frame_table(self, frames, accel=False):
        """frames: items ("body" | "site", name_or_id[, ref=("body" | "site", name_or_id)][, local=True]) — the options as a dict behind
        the two entries, or a dict(type=, id=, ref=, local=) — or a capi.Frame array already resolved; names are resolved once per distinct
        list (the table is kept).  accel: the items of frame_accel — local= and proper=, no ref="""
        if isinstance(frames, C.Array) and frames._type_ is capi.Frame:
            return frames
        what = "frame_accel" if accel else "frame_state"
        key = (what, repr(frames))
        cache = self.__dict__.setdefault("_frame_cache", {})
        if key in cache:
            return cache[key]
        tab = (capi.Frame * len(frames))()
        for k, it in enumerate(frames):
            if isinstance(it, dict):
                head, opt = (it["type"], it["id"]), {a: b for a, b in it.items() if a not in ("type", "id")}
            else:
                head, opt = tuple(it[:2]), dict(it[2]) if len(it) > 2 else {}
            unknown = set(opt) - ({"local", "proper"} if accel else {"ref", "local"})
            if unknown:
                raise MjhError(f"{what}: unknown frame option {sorted(unknown)}")
            tab[k].objtype, tab[k].id = self._frame_id(head, what)
            tab[k].reftype, tab[k].refid = (0, -1) if opt.get("ref") is None else self._frame_id(opt["ref"], what + " ref")
            tab[k].flags = (capi.MJH_FRAME_LOCAL if opt.get("local") else 0) | (capi.MJH_FRAME_PROPER if opt.get("proper") else 0)
        cache[key] = tab
        return tab

    def frame_state(self, frames, env0=0, n=None, jacobian=False):
        """world (or ref-relative) pose and twist of bodies and sites at the envs' present qpos / qvel: dict of float64 arrays pos [n, nframe, 3],
        quat [n, nframe, 4] (w first), linvel, angvel [n, nframe, 3] and, with jacobian=True, jacp, jacr [n, nframe, 3, nv] (world axes, at the
        frame's world origin).  frames: see _frame_table, e.g. [("body", "base"), ("site", "tip", dict(ref=("body", "base"))), ("site", 2, dict(local=True))]"""
        n = self.nenv - env0 if n is None else n
        tab = self._frame_table(frames)
        nf = len(tab)
        st = np.zeros((n, nf, 13)); jac = np.zeros((n, nf, 6, self.nv)) if jacobian else None
        _chk(self.lib, self.lib.mjh_frame_state(self.h, env0, n, nf, C.cast(tab, C.c_void_p), capi.dptr(st), capi.dptr(jac)), "mjh_frame_state")
        out = dict(pos=st[..., 0:3].copy(), quat=st[..., 3:7].copy(), linvel=st[..., 7:10].copy(), angvel=st[..., 10:13].copy())
        if jacobian:
            out["jacp"] = jac[:, :, 0:3].copy(); out["jacr"] = jac[:, :, 3:6].copy()
        return out

    def frame_state_device(self, d_state, d_jac, frames, env0=0, n=None):
        """mjh_frame_state_device: device addresses (data_ptr()) of fp32 state [n, nframe, 13] and Jacobian [n, nframe, 6, nv] (d_jac may be
        None); enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        tab = self._frame_table(frames)
        _chk(self.lib, self.lib.mjh_frame_state_device(self.h, env0, n, len(tab), C.cast(tab, C.c_void_p), C.c_void_p(d_state), C.c_void_p(d_jac)),
             "mjh_frame_state_device")

    # ---- frame accelerations: accelerometer readings and Jdot qvel of bodies and sites (mjh_frame_accel)
    def frame_accel(self, frames, env0=0, n=None, bias=False):
        """classical acceleration J qacc + Jdot qvel of bodies and sites at the envs' present qpos / qvel and the qacc of the last solve: dict
        of float64 arrays linacc, angacc [n, nframe, 3] and, with bias=True, biasp, biasr [n, nframe, 3] (Jdot qvel, always world axes).
        frames: as frame_state's without ref, options local= (the frame's own axes) and proper= (gravity subtracted: an accelerometer),
        e.g. [("site", "imu", dict(local=True, proper=True)), ("body", "hand")]"""
        n = self.nenv - env0 if n is None else n
        tab = self._frame_table(frames, accel=True)
        nf = len(tab)
        acc = np.zeros((n, nf, 6)); bs = np.zeros((n, nf, 6)) if bias else None
        _chk(self.lib, self.lib.mjh_frame_accel(self.h, env0, n, nf, C.cast(tab, C.c_void_p), capi.dptr(acc), capi.dptr(bs)), "mjh_frame_accel")
        out = dict(linacc=acc[..., 0:3].copy(), angacc=acc[..., 3:6].copy())
        if bias:
            out["biasp"] = bs[..., 0:3].copy(); out["biasr"] = bs[..., 3:6].copy()
        return out

    def frame_accel_device(self, d_acc, d_bias, frames, env0=0, n=None):
        """mjh_frame_accel_device: device addresses (data_ptr()) of fp32 acc [n, nframe, 6] and bias [n, nframe, 6] (d_bias may be None);
        enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        tab = self._frame_table(frames, accel=True)
        _chk(self.lib, self.lib.mjh_frame_accel_device(self.h, env0, n, len(tab), C.cast(tab, C.c_void_p), C.c_void_p(d_acc), C.c_void_p(d_bias)),
             "mjh_frame_accel_device")

    def imu(self, sites, env0=0, n=None):
        """IMU readings at `sites` (names or ids): dict of quat [n, nsite, 4] (world orientation, w first), gyro [n, nsite, 3] (angular
        velocity in the site's axes) and accel [n, nsite, 3] (proper acceleration in the site's axes: MuJoCo's <accelerometer>) — one
        frame_state call with local=True and one frame_accel call with local=True, proper=True"""
        sites = list(sites)
        st = self.frame_state([("site", s, dict(local=True)) for s in sites], env0=env0, n=n)
        ac = self.frame_accel([("site", s, dict(local=True, proper=True)) for s in sites], env0=env0, n=n)
        return dict(quat=st["quat"], gyro=st["angvel"], accel=ac["linacc"])

    def mulM(self, vec, env0=0):
        v = np.ascontiguousarray(vec, dtype=np.float64).reshape(-1, self.nv); r = np.zeros_like(v)
        _chk(self.lib, self.lib.mjh_mulM(self.h, env0, v.shape[0], capi.dptr(v), capi.dptr(r)), "mjh_mulM")
        return r

    def set_xfrc_applied(self, xfrc, env0=0):
        """d->xfrc_applied: [n, nbody, 6] force + torque per body at its centre of mass, world frame"""
        x = np.ascontiguousarray(xfrc, dtype=np.float64).reshape(-1, 6 * self.nbody)
        _chk(self.lib, self.lib.mjh_set_xfrc_applied(self.h, env0, x.shape[0], capi.dptr(x)), "mjh_set_xfrc_applied")

    def get_xfrc_applied(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        out = np.zeros((n, self.nbody, 6))
        _chk(self.lib, self.lib.mjh_get_xfrc_applied(self.h, env0, n, capi.dptr(out)), "mjh_get_xfrc_applied")
        return out

    def get_sensordata(self, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        out = np.zeros((n, self.model.nsensordata))
        _chk(self.lib, self.lib.mjh_get_sensordata(self.h, env0, n, capi.dptr(out)), "mjh_get_sensordata")
        return out

    def set_mocap_pose(self, mocapid, pos=None, quat=None, env0=0):
        p = None if pos is None else np.ascontiguousarray(pos, dtype=np.float64).reshape(-1, 3)
        q = None if quat is None else np.ascontiguousarray(quat, dtype=np.float64).reshape(-1, 4)
        n = (p if p is not None else q).shape[0]
        _chk(self.lib, self.lib.mjh_set_mocap_pose(self.h, env0, n, mocapid, capi.dptr(p), capi.dptr(q)), "mjh_set_mocap_pose")

    def set_env_param(self, name, values, env0=0):
        v = np.ascontiguousarray(values, dtype=np.float64)
        v = v.reshape(v.shape[0], -1)
        _chk(self.lib, self.lib.mjh_set_env_param(self.h, EP[name], env0, v.shape[0], capi.dptr(v)), "mjh_set_env_param")

    def set_initial_qpos(self, qpos, env0=0):
        q = np.ascontiguousarray(qpos, dtype=np.float64).reshape(-1, self.nq)
        _chk(self.lib, self.lib.mjh_set_initial_qpos(self.h, env0, q.shape[0], capi.dptr(q)), "mjh_set_initial_qpos")

    def reset(self, env_ids=None):
        if env_ids is None:
            _chk(self.lib, self.lib.mjh_reset(self.h, None, 0), "mjh_reset")
        else:
            ids = np.ascontiguousarray(env_ids, dtype=np.int32)
            _chk(self.lib, self.lib.mjh_reset(self.h, capi.iptr(ids), ids.shape[0]), "mjh_reset")

    # ---- the loop on the device (mjh_*_device of the control side): actions, joint state and resets between device buffers and the engine.
    # Every buffer is an integer device address (taken as is) or an object with data_ptr() such as a torch tensor (checked: device_buffer);
    # dense fp32 rows [n, width], row i = env env0 + i.  The calls are enqueued on the engine's stream and wait for nothing: the caller orders
    # the producer / consumer of a buffer on that stream and keeps the buffer alive until the stream has passed the call.
    def _device_rows(self, what, env0, n, bufs):
        """bufs: (argument name, buffer, row width, dtypes) each -> (n, addresses as c_void_p); n: the rows of the first tensor given, else
        nenv - env0"""
        if n is None:
            n = next((r for r in (_buffer_rows(b, w) for _, b, w, _ in bufs) if r is not None), self.nenv - env0)
        n = int(n)
        return n, [C.c_void_p(device_buffer(b, f"{what}: {name}", n * w, self.device, dt)) for name, b, w, dt in bufs]

    def set_cmd_device(self, ddq=None, dq=None, env0=0, n=None):
        """mjh_set_cmd_device: fp32 ddq / dq [n, nv] on the device (either may be None)"""
        f = ("float32",)
        n, p = self._device_rows("set_cmd_device", env0, n, [("ddq", ddq, self.nv, f), ("dq", dq, self.nv, f)])
        _chk(self.lib, self.lib.mjh_set_cmd_device(self.h, env0, n, p[0], p[1]), "mjh_set_cmd_device")

    def set_pd_target_device(self, target, env0=0, n=None):
        """mjh_set_pd_target_device: fp32 targets [n, nv] on the device"""
        n, p = self._device_rows("set_pd_target_device", env0, n, [("target", target, self.nv, ("float32",))])
        _chk(self.lib, self.lib.mjh_set_pd_target_device(self.h, env0, n, p[0]), "mjh_set_pd_target_device")

    def set_xfrc_applied_device(self, xfrc, env0=0, n=None):
        """mjh_set_xfrc_applied_device: fp32 force + torque per body [n, nbody, 6] on the device"""
        n, p = self._device_rows("set_xfrc_applied_device", env0, n, [("xfrc", xfrc, 6 * self.nbody, ("float32",))])
        _chk(self.lib, self.lib.mjh_set_xfrc_applied_device(self.h, env0, n, p[0]), "mjh_set_xfrc_applied_device")

    def get_joint_state_device(self, qpos=None, qvel=None, qfrc_inverse=None, env0=0, n=None):
        """mjh_get_joint_state_device: fills fp32 qpos [n, nq], qvel [n, nv], qfrc_inverse [n, nv] on the device (any may be None)"""
        f = ("float32",)
        n, p = self._device_rows("get_joint_state_device", env0, n,
                                 [("qpos", qpos, self.nq, f), ("qvel", qvel, self.nv, f), ("qfrc_inverse", qfrc_inverse, self.nv, f)])
        _chk(self.lib, self.lib.mjh_get_joint_state_device(self.h, env0, n, p[0], p[1], p[2]), "mjh_get_joint_state_device")

    def reset_device(self, mask=None, qpos=None, qvel=None, env0=0, n=None):
        """mjh_reset_device: resets the envs of [env0, env0 + n) whose mask byte (uint8 / bool [n]) is not zero (mask None: all of them); a
        selected env takes its row of fp32 qpos [n, nq] / qvel [n, nv] where given, else its initial qpos / zero"""
        f = ("float32",)
        n, p = self._device_rows("reset_device", env0, n,
                                 [("mask", mask, 1, ("uint8", "bool")), ("qpos", qpos, self.nq, f), ("qvel", qvel, self.nv, f)])
        _chk(self.lib, self.lib.mjh_reset_device(self.h, env0, n, p[0], p[1], p[2]), "mjh_reset_device")

    def transplant_state_from(self, other, full_qpos=True):
        """add_old_state() (mj_sim.cpp:465-558): name-matched copy of the per-body state of `other` into this engine"""
        return _chk(self.lib, self.lib.mjh_transplant_state(other.h, self.h, int(bool(full_qpos))), "mjh_transplant_state")

    def set_slot_active(self, body, active, env0=0, n=None):
        n = self.nenv - env0 if n is None else n
        _chk(self.lib, self.lib.mjh_set_slot_active(self.h, env0, n, body, int(active)), "mjh_set_slot_active")

    def spawn_objects(self, envs, bodies, pos, quat=None, vel=None):
        """batched spawn service: n (env, body) pairs, pose [n,3] / [n,4] and twist [n,6] in one call"""
        ev = np.ascontiguousarray(envs, dtype=np.int32); bd = np.ascontiguousarray(bodies, dtype=np.int32)
        a = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (pos, quat, vel)]
        _chk(self.lib, self.lib.mjh_spawn_objects(self.h, len(ev), capi.iptr(ev), capi.iptr(bd), *[capi.dptr(x) for x in a]), "mjh_spawn_objects")

    def destroy_objects(self, envs, bodies):
        ev = np.ascontiguousarray(envs, dtype=np.int32); bd = np.ascontiguousarray(bodies, dtype=np.int32)
        _chk(self.lib, self.lib.mjh_destroy_objects(self.h, len(ev), capi.iptr(ev), capi.iptr(bd)), "mjh_destroy_objects")

    def set_body_pose(self, env, body, pos, quat=None, vel=None):
        a = [None if x is None else np.ascontiguousarray(x, dtype=np.float64) for x in (pos, quat, vel)]
        _chk(self.lib, self.lib.mjh_set_body_pose(self.h, env, body, *[capi.dptr(x) for x in a]), "mjh_set_body_pose")

    # ---- ray casting (mj_ray for every env)
    def _ray_options(self, per_env, options):
        o = capi.RayOptions()
        self.lib.mjh_ray_default_options(C.byref(o))
        o.per_env = int(per_env)
        for k, v in options.items():
            if k not in ("site", "bodyexclude", "flg_static", "cutoff"):
                raise TypeError(f"unknown ray option {k!r}")
            setattr(o, k, v)
        return o

    @property
    def ray_mesh_mode(self):
        """how rays treat mesh geoms: 0 (default) invisible, 1 hit as the convex hull of the kept vertices (mjh_ray_set_mesh_mode)"""
        return self.lib.mjh_ray_get_mesh_mode(self.h)

    @ray_mesh_mode.setter
    def ray_mesh_mode(self, mode):
        _chk(self.lib, self.lib.mjh_ray_set_mesh_mode(self.h, int(mode)), "mjh_ray_set_mesh_mode")

    @property
    def ray_mesh_surface(self):
        """what a visible mesh geom is to a ray: 0 (default) its convex hull, 1 the mesh's own triangles where the asset has any
        (mjh_ray_set_mesh_surface); rays and depth images both obey it"""
        return self.lib.mjh_ray_get_mesh_surface(self.h)

    @ray_mesh_surface.setter
    def ray_mesh_surface(self, surface):
        _chk(self.lib, self.lib.mjh_ray_set_mesh_surface(self.h, int(surface)), "mjh_ray_set_mesh_surface")

    def ray(self, pnt, vec, env0=0, n=None, **options):
        """rays pnt + x vec against the geoms of envs [env0, env0 + n): [nray, 3] arrays are one ray set shared by all envs, [n, nray, 3]
        arrays one set per env.  options: site, bodyexclude, flg_static, cutoff (mjh_ray_options).
        -> (dist [n, nray] float64 in units of |vec|, geomid [n, nray] int32); a miss is (-1, -1)"""
        n = self.nenv - env0 if n is None else n
        p = np.ascontiguousarray(pnt, dtype=np.float64); v = np.ascontiguousarray(vec, dtype=np.float64)
        per_env = p.ndim == 3
        if p.shape != v.shape or p.shape[-1] != 3 or (per_env and p.shape[0] != n):
            raise ValueError("pnt / vec must both be [nray, 3] or [n, nray, 3]")
        nray = p.shape[-2] if p.ndim >= 2 else 1
        o = self._ray_options(per_env, options)
        dist = np.zeros((n, nray)); gid = np.zeros((n, nray), dtype=np.int32)
        _chk(self.lib, self.lib.mjh_ray(self.h, env0, n, nray, capi.dptr(p), capi.dptr(v), C.byref(o), capi.dptr(dist), capi.iptr(gid)), "mjh_ray")
        return dist, gid

    def ray_device(self, d_pnt, d_vec, d_dist, d_geomid, nray, env0=0, n=None, per_env=False, **options):
        """mjh_ray_device: device addresses (data_ptr()) of fp32 pnt / vec [nray, 3] (per_env: [n, nray, 3]), fp32 dist and int32 geomid
        [n, nray]; enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        o = self._ray_options(per_env, options)
        _chk(self.lib, self.lib.mjh_ray_device(self.h, env0, n, int(nray), C.c_void_p(d_pnt), C.c_void_p(d_vec), C.byref(o),
                                               C.c_void_p(d_dist), C.c_void_p(d_geomid)), "mjh_ray_device")

    # ---- depth images (a camera of the model, every env)
    def _depth_options(self, camera, width, height, options):
        o = capi.DepthOptions()
        self.lib.mjh_depth_default_options(C.byref(o))
        if isinstance(camera, str):
            cid = self.lib.mjh_name2id(self.model.ptr, 5, camera.encode())
            if cid < 0:
                raise ValueError(f"no camera named {camera!r}")
            camera = cid
        o.camera = int(camera); o.width = int(width); o.height = int(height)
        for k, v in options.items():
            if k not in ("bodyexclude", "flg_static", "range", "cull", "cutoff"):
                raise TypeError(f"unknown depth option {k!r}")
            setattr(o, k, v)
        return o

    def depth(self, camera, width, height, env0=0, n=None, **options):
        """what camera `camera` (id or name) sees in envs [env0, env0 + n).  options: bodyexclude, flg_static, range, cull, cutoff
        (mjh_depth_options).  -> (depth [n, height, width] float32, geomid [n, height, width] int32); a miss is (-1, -1)"""
        n = self.nenv - env0 if n is None else n
        o = self._depth_options(camera, width, height, options)
        shape = (max(n, 0), max(o.height, 0), max(o.width, 0))
        depth = np.zeros(shape, dtype=np.float32); gid = np.zeros(shape, dtype=np.int32)
        _chk(self.lib, self.lib.mjh_depth(self.h, env0, n, C.byref(o), C.c_void_p(depth.ctypes.data), C.c_void_p(gid.ctypes.data)), "mjh_depth")
        return depth, gid

    def depth_device(self, d_depth, d_geomid, camera, width, height, env0=0, n=None, **options):
        """mjh_depth_device: device addresses (data_ptr()) of fp32 depth and int32 geomid [n, height, width] (d_geomid may be None);
        enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        o = self._depth_options(camera, width, height, options)
        _chk(self.lib, self.lib.mjh_depth_device(self.h, env0, n, C.byref(o), C.c_void_p(d_depth), C.c_void_p(d_geomid)), "mjh_depth_device")

    # ---- lidar range images (a site of the model, every env)
    def _scan_options(self, site, width, height, azimuth, elevation, options):
        """-> (mjh_scan_options, the array that backs its elevation table: to be kept alive over the call)"""
        o = capi.ScanOptions()
        self.lib.mjh_scan_default_options(C.byref(o))
        if isinstance(site, str):
            sid = self.lib.mjh_name2id(self.model.ptr, 3, site.encode())
            if sid < 0:
                raise ValueError(f"no site named {site!r}")
            site = sid
        o.site = -1 if site is None else int(site); o.width = int(width); o.height = int(height)
        if azimuth is not None:
            o.azimuth0, o.azimuth_step = float(azimuth[0]), float(azimuth[1])
        table = None
        if isinstance(elevation, tuple):
            if len(elevation) != 2:
                raise ValueError("elevation is (elevation0, elevation_step) or an array of `height` angles")
            o.elevation0, o.elevation_step = float(elevation[0]), float(elevation[1])
        elif elevation is not None:
            table = np.ascontiguousarray(elevation, dtype=np.float64).reshape(-1)
            if table.size != o.height:
                raise ValueError("the elevation table needs `height` entries")
            o.elevation = capi.dptr(table)
        for k, v in options.items():
            if k not in ("bodyexclude", "flg_static", "cull", "cutoff"):
                raise TypeError(f"unknown scan option {k!r}")
            setattr(o, k, v)
        return o, table

    def scan(self, site, width, height, azimuth=None, elevation=None, env0=0, n=None, points=False, **options):
        """the lidar scan from site `site` (id or name; None / -1: the world frame) in envs [env0, env0 + n): `width` columns at azimuth
        azimuth[0] + j azimuth[1] and `height` rows at elevation[0] + i elevation[1] (a tuple) or at the angles of an array, radians.
        options: bodyexclude, flg_static, cull, cutoff (mjh_scan_options).
        -> (range [n, height, width] float32, geomid [n, height, width] int32[, points [n, height, width, 3] float32 in the sensor
        frame]); a miss is (-1, -1[, (0, 0, 0)])"""
        n = self.nenv - env0 if n is None else n
        o, table = self._scan_options(site, width, height, azimuth, elevation, options)
        shape = (max(n, 0), max(o.height, 0), max(o.width, 0))
        rng = np.zeros(shape, dtype=np.float32); gid = np.zeros(shape, dtype=np.int32)
        pts = np.zeros(shape + (3,), dtype=np.float32) if points else None
        _chk(self.lib, self.lib.mjh_scan(self.h, env0, n, C.byref(o), C.c_void_p(rng.ctypes.data), C.c_void_p(gid.ctypes.data),
                                         C.c_void_p(pts.ctypes.data) if points else None), "mjh_scan")
        return (rng, gid, pts) if points else (rng, gid)

    def scan_device(self, d_range, d_geomid, d_points, site, width, height, azimuth=None, elevation=None, env0=0, n=None, **options):
        """mjh_scan_device: device addresses (data_ptr()) of fp32 range and int32 geomid [n, height, width] and fp32 points
        [n, height, width, 3] (d_geomid and d_points may be None); enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        o, table = self._scan_options(site, width, height, azimuth, elevation, options)
        _chk(self.lib, self.lib.mjh_scan_device(self.h, env0, n, C.byref(o), C.c_void_p(d_range), C.c_void_p(d_geomid), C.c_void_p(d_points)), "mjh_scan_device")

    # ---- height scans (a grid of parallel rays under a site of the model, every env)
    _HSCAN_ALIGN = {"yaw": 0, "base": 1, "world": 2}

    def _heightscan_options(self, site, width, height, spacing, offset, above, align, options):
        o = capi.HeightScanOptions()
        self.lib.mjh_heightscan_default_options(C.byref(o))
        if isinstance(site, str):
            sid = self.lib.mjh_name2id(self.model.ptr, 3, site.encode())
            if sid < 0:
                raise ValueError(f"no site named {site!r}")
            site = sid
        if align not in self._HSCAN_ALIGN:
            raise ValueError('align is "yaw", "base" or "world"')
        spacing = (spacing, spacing) if np.isscalar(spacing) else tuple(spacing)
        if len(spacing) != 2 or len(offset) != 2:
            raise ValueError("spacing and offset are (x, y) pairs")
        o.site = -1 if site is None else int(site); o.align = self._HSCAN_ALIGN[align]; o.width = int(width); o.height = int(height)
        o.spacing[0], o.spacing[1] = float(spacing[0]), float(spacing[1])
        o.offset[0], o.offset[1] = float(offset[0]), float(offset[1])
        o.above = float(above)
        for k, v in options.items():
            if k not in ("bodyexclude", "exclude_tree", "flg_static", "cull", "cutoff"):
                raise TypeError(f"unknown height-scan option {k!r}")
            setattr(o, k, v)
        return o

    def height_scan(self, site, width, height, spacing, offset=(0, 0), above=1.0, align="yaw", env0=0, n=None, points=False, **options):
        """the height scan under site `site` (id or name; None / -1: the world frame) in envs [env0, env0 + n): a `height` x `width` grid
        of parallel rays, cell (i, j) at offset + ((j, i) - ((width, height) - 1) / 2) * spacing in the grid frame, cast from `above`
        along the grid's -z.  align: "yaw" (the grid follows the site's heading, the rays go along the world's -z), "base" (the
        site's own frame) or "world".  spacing: (x, y) or one number.  options: bodyexclude, exclude_tree, flg_static, cull, cutoff
        (mjh_heightscan_options).
        -> (range [n, height, width] float32, geomid [n, height, width] int32[, points [n, height, width, 3] float32 in the grid
        frame: (x, y, above - range)]); a miss is (-1, -1[, the ray's start point])"""
        n = self.nenv - env0 if n is None else n
        o = self._heightscan_options(site, width, height, spacing, offset, above, align, options)
        shape = (max(n, 0), max(o.height, 0), max(o.width, 0))
        rng = np.zeros(shape, dtype=np.float32); gid = np.zeros(shape, dtype=np.int32)
        pts = np.zeros(shape + (3,), dtype=np.float32) if points else None
        _chk(self.lib, self.lib.mjh_heightscan(self.h, env0, n, C.byref(o), C.c_void_p(rng.ctypes.data), C.c_void_p(gid.ctypes.data),
                                               C.c_void_p(pts.ctypes.data) if points else None), "mjh_heightscan")
        return (rng, gid, pts) if points else (rng, gid)

    def height_scan_device(self, d_range, d_geomid, d_points, site, width, height, spacing, offset=(0, 0), above=1.0, align="yaw", env0=0, n=None, **options):
        """mjh_heightscan_device: device addresses (data_ptr()) of fp32 range and int32 geomid [n, height, width] and fp32 points
        [n, height, width, 3] (d_geomid and d_points may be None); enqueued on the engine's stream, valid after synchronize()"""
        n = self.nenv - env0 if n is None else n
        o = self._heightscan_options(site, width, height, spacing, offset, above, align, options)
        _chk(self.lib, self.lib.mjh_heightscan_device(self.h, env0, n, C.byref(o), C.c_void_p(d_range), C.c_void_p(d_geomid), C.c_void_p(d_points)), "mjh_heightscan_device")

    # ---- RGB-D images: depth, geom id, world-frame normal, shaded colour
    def _render_options(self, camera, width, height, options):
        o = capi.RenderOptions()
        self.lib.mjh_render_default_options(C.byref(o))
        shading = {k: options.pop(k) for k in ("ambient", "diffuse", "background") if k in options}
        o.view = self._depth_options(camera, width, height, options)
        if "ambient" in shading:
            o.ambient = float(shading["ambient"])
        if "diffuse" in shading:
            o.diffuse = float(shading["diffuse"])
        if "background" in shading:
            bg = [float(x) for x in shading["background"]]
            if len(bg) != 4:
                raise ValueError("background needs four components")
            o.background = (C.c_float * 4)(*bg)
        return o

    def render(self, camera, width, height, env0=0, n=None, normal=True, rgba=True, **options):
        """what camera `camera` (id or name) sees in envs [env0, env0 + n), with surface normals and colour.  options: mjh_depth_options'
        and ambient, diffuse, background (mjh_render_options).  -> (depth [n, height, width] float32, geomid [n, height, width] int32,
        normal [n, height, width, 3] float32 (world frame, towards the camera; None unless asked for), rgba [n, height, width, 4]
        uint8 (None unless asked for)); a miss is (-1, -1, (0, 0, 0), background)"""
        n = self.nenv - env0 if n is None else n
        o = self._render_options(camera, width, height, dict(options))
        shape = (max(n, 0), max(o.view.height, 0), max(o.view.width, 0))
        depth = np.zeros(shape, dtype=np.float32); gid = np.zeros(shape, dtype=np.int32)
        nrm = np.zeros(shape + (3,), dtype=np.float32) if normal else None
        col = np.zeros(shape + (4,), dtype=np.uint8) if rgba else None
        _chk(self.lib, self.lib.mjh_render(self.h, env0, n, C.byref(o), C.c_void_p(depth.ctypes.data), C.c_void_p(gid.ctypes.data),
                                           C.c_void_p(nrm.ctypes.data) if normal else None, C.c_void_p(col.ctypes.data) if rgba else None), "mjh_render")
        return depth, gid, nrm, col

    def render_device(self, d_depth, d_geomid, d_normal, d_rgba, camera, width, height, env0=0, n=None, **options):
        """mjh_render_device: device addresses (data_ptr()) of fp32 depth and int32 geomid [n, height, width], fp32 normal
        [n, height, width, 3] and uint8 rgba [n, height, width, 4]; any may be None, not all; enqueued on the engine's stream, valid
        after synchronize()"""
        n = self.nenv - env0 if n is None else n
        o = self._render_options(camera, width, height, dict(options))
        _chk(self.lib, self.lib.mjh_render_device(self.h, env0, n, C.byref(o), C.c_void_p(d_depth), C.c_void_p(d_geomid),
                                                  C.c_void_p(d_normal), C.c_void_p(d_rgba)), "mjh_render_device")

    # ---- lights and cast shadows in the colour image
    @property
    def render_lighting(self):
        """0: the colour image is shaded by the headlight alone (the default); 1: it also takes the model's active lights
        (mjh_render_set_lighting)"""
        return self.lib.mjh_render_get_lighting(self.h)

    @render_lighting.setter
    def render_lighting(self, mode):
        _chk(self.lib, self.lib.mjh_render_set_lighting(self.h, int(mode)), "mjh_render_set_lighting")

    @property
    def light_options(self):
        """dict(shadows, cull, bias) of mjh_light_options; assign a dict with any of the three keys"""
        o = capi.LightOptions()
        _chk(self.lib, self.lib.mjh_render_get_light_options(self.h, C.byref(o)), "mjh_render_get_light_options")
        return {"shadows": o.shadows, "cull": o.cull, "bias": o.bias}

    @light_options.setter
    def light_options(self, options):
        cur = self.light_options
        for k in options:
            if k not in cur:
                raise TypeError(f"unknown light option {k!r}")
        cur.update(options)
        o = capi.LightOptions(int(cur["shadows"]), int(cur["cull"]), float(cur["bias"]))
        _chk(self.lib, self.lib.mjh_render_set_light_options(self.h, C.byref(o)), "mjh_render_set_light_options")

    # ---- textures in the colour image
    @property
    def render_texturing(self):
        """0: a geom's base colour is its geom_rgba (the default); 1: where the geom carries a texture the base colour is geom_rgba
        times the texel sampled at the hit point (mjh_render_set_texturing)"""
        return self.lib.mjh_render_get_texturing(self.h)

    @render_texturing.setter
    def render_texturing(self, mode):
        _chk(self.lib, self.lib.mjh_render_set_texturing(self.h, int(mode)), "mjh_render_set_texturing")

    def set_light_active(self, light, on):
        """switch light `light` (id or name) for every env of the engine, from the next render call on"""
        if isinstance(light, (str, bytes)):
            name = light.encode() if isinstance(light, str) else light
            light = self.lib.mjh_name2id(self.lib.mjh_engine_model(self.h), 6, name)
        _chk(self.lib, self.lib.mjh_set_light_active(self.h, int(light), int(bool(on))), "mjh_set_light_active")

    def export_state_device(self, device_ptr):
        _chk(self.lib, self.lib.mjh_export_state_device(self.h, C.c_void_p(device_ptr)), "mjh_export_state_device")

    @property
    def state_stride(self):
        return self.lib.mjh_state_stride(self.h)

    @property
    def lds_bytes(self):
        return self.lib.mjh_lds_bytes(self.h)

    def solver_order(self):
        """2: mj_solPGS's row order (default); legacy: 1 contact patches, 0 independent pairs / groups of blocks (mjh_solver_order)"""
        return self.lib.mjh_solver_order(self.h)

    def patch_sweep(self):
        """1: contact-patch form of the sweeps (small free-body models), 0: a block form (mjh_patch_sweep)"""
        return self.lib.mjh_patch_sweep(self.h)

    def window_solver(self):
        """1: mjh_step = assemble launch + mjh_window_kernel (four envs per wavefront, rows in registers), 0: one fused launch"""
        return self.lib.mjh_window_solver(self.h)

    def pgs_schedule(self):
        """1: row order, list-scheduled (default), 2: row order, strictly sequential, 0: legacy reordering schedule (mjh_pgs_schedule)"""
        return self.lib.mjh_pgs_schedule(self.h)

    def dense_solver(self):
        """1: articulated many-body model solved by the dense row-space solver (mjh_dense_solver)"""
        return self.lib.mjh_dense_solver(self.h)

    def load_tables(self, t):
        """apply per-env parameter tables + initial poses (dict as returned by *_randomize) and reset"""
        for k in ["geom_size", "geom_rbound", "body_mass", "body_inertia", "body_invweight0", "dof_invweight0"]:
            self.set_env_param(k, t[k])
        self.set_initial_qpos(t["qpos"])
        self.reset()
        return t

    def load_s24(self, seed_base=0x5EED0000, env_offset=0):
        """Apply the per-env S24 randomisation (sizes, masses, initial poses) and reset."""
        t = self.model.s24_randomize(env_offset, self.nenv, seed_base)
        for k in ["geom_size", "geom_rbound", "body_mass", "body_inertia", "body_invweight0", "dof_invweight0"]:
            self.set_env_param(k, t[k])
        self.set_initial_qpos(t["qpos"])
        self.reset()
        return t


class Group:
    """mjh_group: the environments of one simulation sharded over the GPUs of a node (one engine + stream per device, env ranges
    contiguous); the only exchange is publish() = pack + RCCL all-gather of the state slice (include/mjhip.h "multi-GPU")."""

    def __init__(self, model, nenv_total, devices):
        self.lib = model.lib; self.model = model; self.nenv = nenv_total
        dv = np.ascontiguousarray(devices, dtype=np.int32)
        h = C.c_void_p()
        _chk(self.lib, self.lib.mjh_group_create(model.ptr, nenv_total, capi.iptr(dv), len(dv), C.byref(h)), "mjh_group_create")
        self.h = h
        self.ndev = self.lib.mjh_group_ndev(h)
        self.ranges = []
        self.engines = []
        for k in range(self.ndev):
            a, b = C.c_int(0), C.c_int(0)
            _chk(self.lib, self.lib.mjh_group_env_range(h, k, C.byref(a), C.byref(b)), "mjh_group_env_range")
            self.ranges.append((a.value, b.value))
            self.engines.append(Engine.from_handle(model, self.lib.mjh_group_engine(h, k), b.value, int(dv[k])))
        self.stride = self.lib.mjh_group_state_stride(h)

    @property
    def uses_rccl(self): return bool(self.lib.mjh_group_uses_rccl(self.h))
    def step(self, n=1, with_inverse=False): _chk(self.lib, self.lib.mjh_group_step(self.h, n, int(with_inverse)), "mjh_group_step")
    def step1(self): _chk(self.lib, self.lib.mjh_group_step1(self.h), "mjh_group_step1")
    def inverse(self): _chk(self.lib, self.lib.mjh_group_inverse(self.h), "mjh_group_inverse")
    def step2(self): _chk(self.lib, self.lib.mjh_group_step2(self.h), "mjh_group_step2")
    def synchronize(self): _chk(self.lib, self.lib.mjh_group_synchronize(self.h), "mjh_group_synchronize")

    def publish(self):
        """-> [nenv, 1 + nq + nv] float32: time | qpos | qvel of every env in env order (device 0's copy of the all-gather)"""
        out = np.zeros((self.nenv, self.stride), dtype=np.float32)
        _chk(self.lib, self.lib.mjh_group_publish(self.h, out.ctypes.data_as(C.POINTER(C.c_float))), "mjh_group_publish")
        return out

    def publish_device(self):
        """pack + all-gather without the host copy (the gathered state stays on every device: mjh_group_state_device)"""
        _chk(self.lib, self.lib.mjh_group_publish(self.h, None), "mjh_group_publish")

    def wait_publish(self, rank, stream=None):
        _chk(self.lib, self.lib.mjh_group_wait_publish(self.h, int(rank), C.c_void_p(stream or 0)), "mjh_group_wait_publish")

    def release_publish(self, rank, stream=None):
        """the consumer on `stream` is done reading device `rank`'s gathered state: the next publish may overwrite it"""
        _chk(self.lib, self.lib.mjh_group_release_publish(self.h, int(rank), C.c_void_p(stream or 0)), "mjh_group_release_publish")

    def set_publish_timing(self, on=True): _chk(self.lib, self.lib.mjh_group_set_publish_timing(self.h, int(on)), "mjh_group_set_publish_timing")
    def get_publish_timing(self):
        """-> (mean duration of the exchange [ms], publishes) since the last call"""
        ms_, cnt = C.c_double(0), C.c_int(0)
        _chk(self.lib, self.lib.mjh_group_get_publish_timing(self.h, C.byref(ms_), C.byref(cnt)), "mjh_group_get_publish_timing")
        return ms_.value, cnt.value

    def locate(self, env):
        r, l = C.c_int(0), C.c_int(0)
        _chk(self.lib, self.lib.mjh_group_locate(self.h, env, C.byref(r), C.byref(l)), "mjh_group_locate")
        return r.value, l.value

    def close(self):
        if getattr(self, "h", None):
            for e in self.engines:
                e.close()
            self.lib.mjh_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
