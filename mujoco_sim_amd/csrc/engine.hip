// engine.hip — host side of the C ABI (include/mjhip.h): device model upload, per-env state in
// HBM (env-major fp32 rows padded to 128 B), kernel launches on the caller's HIP stream, and
// double<->float marshalling for the mjData-style getters/setters the reference's ROS layer uses.
// gfx950 only; there is no CPU fallback — every entry point fails loudly without a HIP device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mjhip.h"
#include "step_kernel.h"
#include "dev_ray.h"
#include "dev_depth.h"
#include "dev_scan.h"
#include "dev_heightscan.h"
#include "dev_contact.h"
#include "dev_frame.h"
#include "dev_control.h"
#include "dev_render.h"
#include "dev_light.h"
#include "dev_texture.h"
#include "ray_tables.h"

void mjh_set_error(const std::string& s);  // model_builder.cpp
hipError_t mjh_launch_window(hipStream_t st, int nvt, int grid, size_t lds, const DConst* dC, const DState& S, int env0, int n, int nl, int wxf, int n32, int n64);   // window.hip
hipError_t mjh_dense_attributes(size_t build_lds, size_t solve_lds);   // dense.hip (kernels of dense_pgs.h)
// hfield.hip: the step kernel's instances for models with height-field pairs (every layout) and their LDS ceilings
hipError_t mjh_launch_step_hf(hipStream_t st, int nr, bool diag, int wpre, int grid, size_t lds, const DConst* dC, const DState& S,
                              int env0, int nsteps, int ph, int xflags);
hipError_t mjh_step_hf_attributes(size_t lds);
hipError_t mjh_launch_dense(hipStream_t st, int n, size_t build_lds, size_t solve_lds, const DConst* dC, const DState& S, int env0);
#define DN_CAP_MAX 256          // row capacity of the dense solver (dense_pgs.h)

#define HIPCHK(call)                                                                             \
  do {                                                                                           \
    hipError_t e_ = (call);                                                                      \
    if (e_ != hipSuccess) {                                                                      \
      mjh_set_error(std::string(#call) + ": " + hipGetErrorString(e_));                          \
      return MJH_ERR_NO_DEVICE;                                                                  \
    }                                                                                            \
  } while (0)

// restores the engine's device-state descriptor when a scope that patched it (export pointers, launch order) is left on
// ANY path, early error returns included
struct StateGuard {
  DState* where; DState saved;
  explicit StateGuard(DState* w) : where(w), saved(*w) {}
  ~StateGuard() { *where = saved; }
  StateGuard(const StateGuard&) = delete; StateGuard& operator=(const StateGuard&) = delete;
};
struct DevBuf {   // temporary device allocation freed on every path
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
};

#define MJH_MAX_COHORTS 8
#define MJH_IO_SLOTS 8             // host-mapped staging of mjh_set_cmd: ring of slots ...
#define MJH_IO_PUT_FLOATS 4096     // ... of this many floats each (larger calls take the copy path)
#define MJH_IO_GET_FLOATS 16384    // host-mapped staging of mjh_get_joint_state
// HIP streams that share a hardware queue serialise; the engine uses up to five at once (three cohorts, the caller's stream, the
// export stream) and RCCL adds its own.  The runtime reads GPU_MAX_HW_QUEUES (default 4) when it initialises, i.e. at the first
// HIP call of the process: asked for here, when the library is loaded, unless the host has set it itself.
__attribute__((constructor)) static void mjh_library_init() { setenv("GPU_MAX_HW_QUEUES", "8", 0); }
struct mjh_engine {
  const mjh_model* model = nullptr;
  int nenv = 0, device = 0;
  hipStream_t stream = nullptr;
  DModel M{};
  DState S{};
  Lay L{};
  int lds_bytes = 0, lds_bytes_pre = 0;   // dynamic LDS per env of the step kernel; ... of its assemble-only instance (no patch pool: more envs per CU; HostPack's lds_bytes_wpre)
  DHField H{};                            // height fields (H.has_hfield: every launch of the step kernel takes an HF instance, hfield.hip)
  bool report = false; DReport R{};       // contact report (mjh_set_contact_report when the engine was created): the kernels' descriptor of its buffers
  // per-body contact force (mjh_body_contact_force_device, contact.hip): the selection table of the last call on the device — the pinned host
  // buffer the upload is issued from, the event that marks the upload's end — and the selection it holds; a call with the same one uploads nothing
  int2* csel_tab = nullptr; int2* csel_host = nullptr; int csel_cap = 0; hipEvent_t csel_up = nullptr; std::vector<int> csel_have; float* csel_io = nullptr; size_t csel_io_words = 0;
  DWpre W{};                              // patch models: where the assemble-only instance keeps its base rows and per-base vectors (derive_device_model)
  size_t dense_lds = 0, dense_solve_lds = 0;   // dynamic LDS of mjh_dense_build_kernel / mjh_dense_solve_kernel
  // dense solver on / off per cohort: mjh_order_kernel leaves "an env of the cohort swept long" in a host-mapped word (four slots per
  // cohort, one per rebuild of the launch order); the host adopts the word of TWO rebuilds ago after waiting for that kernel's event
  // (long finished: no stall, and the decision depends on the step count only, not on timing: runs stay reproducible)
  // per-step host traffic of the reference's loop (MjHWInterface::read / write: mjh_get_joint_state / mjh_set_cmd on a few envs): a
  // host-mapped staging area the device reads and writes directly — one small kernel per call instead of two or three pageable 2D
  // copies; the write side is a ring of slots, each fenced by an event, so mjh_set_cmd does not wait for the device
  float* h_io = nullptr; float* d_io = nullptr; hipEvent_t io_ev[MJH_IO_SLOTS] = {}; bool io_used[MJH_IO_SLOTS] = {}; unsigned io_next = 0;
  int win_lean = -1;        // (tests, MJH_WINDOW_LEAN read at creation: 1 / 0 forces the lean / the fat window instance of a model within 256 rows; -1: by the rows seen)
  bool win_straight = true; // (MJH_WINDOW_STRAIGHT read at creation: 0 keeps the lean window instance in its general sweep loop; same values either way)
  int* h_wn = nullptr; int* d_wn = nullptr; int cur_cohort = -1;   // window models: largest row count per cohort (host-mapped, written by mjh_order_kernel); cohort of the launch being issued
  int* h_dense = nullptr; int* d_dense = nullptr; hipEvent_t ev_dense[MJH_MAX_COHORTS][4] = {}; unsigned dense_epoch[MJH_MAX_COHORTS] = {}; bool dense_now[MJH_MAX_COHORTS];
  int* dI = nullptr; float* dF = nullptr; DConst* dC = nullptr;
  std::vector<int> hI;  // host copy of the int tables (controlled / odom are patched in place)
  int o_controlled = 0, o_odom = 0;
  std::vector<void*> allocs;
  float* scratch = nullptr; size_t scratch_floats = 0;  // export staging
  float* p_tables[MJH_EP_COUNT] = {nullptr};
  int* d_order = nullptr;   // LPT launch order (mjh_order_kernel)
  bool lpt = true;
  bool split3 = true;         // many-body layout: three-launch step (MJH_SPLIT3=0: fused kernel)
  bool order_valid = false;   // d_order holds a full-range permutation (split API); mjh_step sorts per cohort
  // one captured graph per cohort and variant of its step chain (mjh_step: assemble -> [dense build -> dense solve] -> solve -> integrate of the
  // many-body layout; assemble -> window kernel of the window chain): the chain is queued with ONE hipGraphLaunch per cohort-step
  struct ChainGraph { hipGraphExec_t exec = nullptr; unsigned char S[sizeof(DState)]; int g0 = -1, n = -1, key = -1; bool nocap = false; };   // nocap: capture / instantiate failed once for this slot — plain launches from then on
  int last_launches = 0;      // queue entries the last mjh_step issued per cohort-step (1: a captured graph; else the chain's kernel launches)
  ChainGraph cgraph[MJH_MAX_COHORTS][8];
  int steps_per_launch = 8;   // mjh_step(n): steps one launch of a loop-capable kernel instance runs (mjh_set_steps_per_launch; 1: one launch per step)
  long order_age = 0; int order_G = 0; int last_chunk = 1;   // last_chunk: steps of the previous launch (the sort is renewed when a multiple of MJH_ORDER_EVERY was crossed)   // mjh_step renews its per-cohort sorts every MJH_ORDER_EVERY-th step; order_G: cohort count they were made for (-1: none)
  // Cohorts: mjh_step() splits the envs into ncohort contiguous groups, each stepped on its own stream, so that the
  // low-occupancy tail of one cohort's step kernel overlaps the next cohort's (or its own next step's) bulk.  The
  // caller's stream forks into the cohort streams at mjh_step and joins them again at the next other API call.
  int ncohort = 1;
  hipStream_t cstream[MJH_MAX_COHORTS] = {nullptr};
  hipEvent_t ev_fork = nullptr, ev_join[MJH_MAX_COHORTS] = {nullptr};
  bool forked = false;
  // optional per-launch timing of the step kernels (mjh_set_launch_timing)
  bool timing = false; int timing_stride = 1; long timing_count = 0;   // every timing_stride-th step launch is bracketed
  std::vector<std::pair<hipEvent_t, hipEvent_t>> tev; size_t tev_used = 0;
  bool step1_done = false;
  bool handover = false;        // window chain: the last step1 [+ inverse] launch left the hand-over mjh_step2 sweeps (dropped by any call that may change what it was built from)
  bool step1_pending = false;   // mjh_step1 has been called, its launch is deferred to the next entry point (fused with mjh_inverse if that is the one)
  // in-engine joint-space PD effort controller (mjh_set_pd_controller): ddq written on the device in front of every step
  float pd_kp = 0, pd_kd = 0; float* pd_target = nullptr; bool pd_on = false;
  // ray casting (mjh_ray / mjh_ray_device, ray.hip): per-geom and per-hfield tables uploaded at the first call, staging of the host form
  int4* ray_ginfo = nullptr; RayHField* ray_hf = nullptr; float* ray_hfdata = nullptr; bool ray_ready = false;
  // mesh mode (mjh_ray_set_mesh_mode): the geom table of mode 1 (mesh geoms typed MJH_GEOM_MESH with their mesh id; the mode-0 table itself
  // in a model without hull planes), the per-mesh table and the fp32 planes — uploaded with the others; a mode change switches tables
  int ray_mesh_mode = 0; int4* ray_ginfo_mesh = nullptr; RayMesh* ray_mesh = nullptr; float4* ray_planes = nullptr;
  // mesh surface (mjh_ray_set_mesh_surface): the third geom table (mesh geoms whose asset has triangles typed RAY_TYPE_TRIMESH; the mode-1
  // table itself in a model without triangles), the per-mesh table, the BVH nodes and the triangle records (ray_bvh.h) — built and
  // uploaded by the first launch issued with the triangles selected, freed with the engine
  int ray_mesh_surface = 0; bool ray_tri_ready = false; std::vector<int4> ray_gi_mesh_host;
  int4* ray_ginfo_tri = nullptr; RayTriMesh* ray_trimesh = nullptr; RayNode* ray_nodes = nullptr; float4* ray_tris = nullptr;
  float* ray_io = nullptr; size_t ray_io_floats = 0;
  // colour images (mjh_render / mjh_render_device, render.hip): geom_rgba as float4 per geom, uploaded at the first render call; the depth
  // and geom-id images of a device-form call whose caller takes neither
  float4* ray_color = nullptr; float* render_io = nullptr; size_t render_io_floats = 0;
  // lights (mjh_render_set_lighting, light.hip): the mode, the options, and the model's lights as the kernel takes them, read from the
  // model once (light_tables); the active mask is applied when a call packs its launch descriptor
  int light_mode = 0; mjh_light_options light_opt = {1, 1, 1e-3f};
  bool lights_ready = false; int nlight = 0; LightRec lights[MJH_MAXLIGHT]; int light_on[MJH_MAXLIGHT];
  // textures (mjh_render_set_texturing, texture.hip): the mode; the geoms' records and the texels, one word each, uploaded at the first
  // textured render call (texture_tables); the texel image of a call
  int tex_mode = 0; TexRec* tex_rec = nullptr; unsigned* tex_data = nullptr; float* tex_io = nullptr; size_t tex_io_floats = 0;
  // lidar scans (mjh_scan / mjh_scan_device, scan.hip): the angle tables of the last call's pattern — the device buffer the kernel reads,
  // the pinned host buffer the upload is issued from (scan_up marks the upload's end: the host buffer is not rewritten before it) —
  // and the pattern they hold; a call with the same pattern uploads nothing
  float* scan_tab = nullptr; size_t scan_tab_floats = 0; float* scan_host = nullptr; size_t scan_host_floats = 0; hipEvent_t scan_up = nullptr;
  bool scan_have = false; int scan_w = 0, scan_h = 0; double scan_az[2] = {0, 0}, scan_el[2] = {0, 0}; bool scan_table = false; std::vector<double> scan_elev;
  // height scans (mjh_heightscan / mjh_heightscan_device, heightscan.hip): the model's body_rootid on the device, uploaded at the first call
  // with exclude_tree = 1 (an engine that never asks has no such buffer)
  int* hscan_root = nullptr;
  // frame states (mjh_frame_state / mjh_frame_state_device, frame.hip): the per-model tables, built and uploaded at the first call (freed with the
  // engine's other allocations); the frame table of the last call on the device — the pinned host buffer the upload is issued from, the event
  // that marks the upload's end — and the frames it holds (a call with the same ones uploads nothing); staging of the host form
  bool frame_ready = false; FrameModel frame_model{};
  struct FrameTable { FrameRec* tab = nullptr; FrameRec* host = nullptr; int cap = 0; hipEvent_t up = nullptr; std::vector<int> have; };
  FrameTable frame_tab;
  float* frame_io = nullptr; size_t frame_io_floats = 0;
  // frame accelerations (mjh_frame_accel / mjh_frame_accel_device, frame_acc.hip): the per-model tables above; a last-call frame table of
  // their own, so that alternating state and acceleration calls upload nothing; staging of the host form
  FrameTable facc_tab;
  float* facc_io = nullptr; size_t facc_io_floats = 0;
  // mjh_reset with an id list (control.hip): the ids of a call go through a ring of pinned slots, each fenced by an event like the slots of
  // mjh_set_cmd, into one device buffer (rewritten in stream order); rid_cap ints per slot, grown to the longest list seen
  int* rid_host = nullptr; int* rid_dev = nullptr; size_t rid_cap = 0; hipEvent_t rid_ev[MJH_IO_SLOTS] = {}; bool rid_used[MJH_IO_SLOTS] = {}; unsigned rid_next = 0;
};

static int pad32(int n) { return ((n + 31) / 32) * 32; }

template <class T> static int dev_alloc(mjh_engine* e, T** p, size_t n, bool zero = true) {
  void* q = nullptr;
  HIPCHK(hipMalloc(&q, std::max<size_t>(n, 1) * sizeof(T)));
  if (zero) HIPCHK(hipMemsetAsync(q, 0, std::max<size_t>(n, 1) * sizeof(T), e->stream));
  e->allocs.push_back(q);
  *p = (T*)q;
  return MJH_OK;
}

// 1 (default): mjh_step queues the many-body layout's launch chain of a cohort-step as one captured graph; 2: the window chain as well (S24:
// 11.42 against 11.63 M env-steps/s with two plain launches — the graph's own launch costs more than it saves there); 0: never
static int g_chain_graph = getenv("MJH_CHAIN_GRAPH") ? atoi(getenv("MJH_CHAIN_GRAPH")) : 1;
extern "C" void mjh_set_chain_graph(int mode) { g_chain_graph = mode < 0 ? 0 : (mode > 2 ? 2 : mode); }

static int ensure_scratch(mjh_engine* e, size_t floats) {
  if (floats <= e->scratch_floats) return MJH_OK;
  if (e->scratch) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->scratch)); }
  HIPCHK(hipMalloc((void**)&e->scratch, floats * sizeof(float)));
  e->scratch_floats = floats;
  return MJH_OK;
}

// models that need the EXTRA kernel instances: generic convex narrow phase (cylinder-x, capsule-box, ellipsoid, mesh) or noslip sweeps
// ... or sites / sensors / mocap bodies / connect-weld equalities; and (engine state) Cartesian forces on bodies in use
static bool extra_instance(const DModel& M) { return M.has_convex || M.noslip_iterations > 0 || M.nsensor > 0 || M.nmocap > 0 || M.has_weld; }

// windows of the window kernel's LDS tier for the next launch of cohort e->cur_cohort
static int window_tier(const mjh_engine* e) {
  static const int nl_env = getenv("MJH_WN_NL") ? atoi(getenv("MJH_WN_NL")) : -1;      // (experiments: force the number of LDS-tier windows)
  // ... and none at all while no env of the cohort comes near the register-resident windows' rows: mjh_order_kernel leaves the cohort's
  // largest row count in a host-mapped word whenever it renews the launch order; read unsynchronised — the tiers hold the same values,
  // the choice changes where a window waits, not what is computed (S24: 9.13 -> 9.35 M env-steps/s; S24D needs the tier)
  const int nwreg = e->M.win_nvt == 24 ? WN_NW24 : WN_NW32;
  const int seen = (e->h_wn && e->cur_cohort >= 0) ? *(volatile int*)(e->h_wn + e->cur_cohort) : (1 << 20);
  const int nl_full = std::min(WN_MAXW, (int)((40 * 1024 - 1024) / (4 * WN_XREC(e->M.win_nvt) * 16 * sizeof(float))));
  // (with the 32-row section on, the 16-row form only meets envs of at most WN32_MIN_ROWS rows — or more than 128, the tier's clients)
  const bool sec32 = e->S.win32 > 0 && e->M.win_nvt == 24 && e->S.win32 <= 16 * nwreg;
  const bool tier = sec32 ? seen > 32 * WN32_NW : seen + 16 > 16 * nwreg;
  // (models whose rows can exceed 256 — win_maxw > 16 — always get the tier: the 64-row section keeps the tiles of its last windows there,
  //  and which envs take that section is decided on the device)
  // Without the tier the launcher takes the LEAN instance (window.hip: 376 registers — an assemble wavefront of another cohort fits on the same SIMD),
  // with it the fat one (424).  Both sweep every env in the same form with the same values, so the lagged word above only picks where windows wait.
  // (tests: MJH_WINDOW_LEAN = 1 / 0 forces the lean / the fat instance for models within 256 rows)
  if (nl_env < 0 && e->win_lean >= 0 && e->M.win_maxw <= 16) return e->win_lean ? 0 : nl_full;
  return nl_env >= 0 ? nl_env : ((tier || e->M.win_maxw > 16) ? nl_full : 0);
}
// wmode (window chain of small free-body models): 0 the whole step; 1 the assemble launch only, every env handed over — the split API's
// mjh_step1 [+ mjh_inverse] doing the work mjh_step2 would otherwise repeat (the rows only exist in LDS); 2 the window kernel only;
// 3 the contact snapshot (mjh_get_contacts) through the assemble-only instance — the collision code the model's steps run —, nothing handed over
static int launch_on(mjh_engine* e, hipStream_t st, int env0, int n, int nsteps, int ph, int xflags, int wmode = 0, int tier_nl = -1) {
  if (n <= 0) return MJH_OK;
  // window sweep (window_pgs.h): every launch that runs mj_step2 to the end (the fused step and the split API's step2) of a small
  // free-body model = assemble launch (PH_PRE), then four envs per wavefront through the sweeps and the integration
  // (wmode 1 may carry XF_PROF: mjh_debug_stage_cycles stamps the assemble-only instance; no window launch follows it)
  const bool snap = wmode == 3 && e->M.window && e->S.wbuf && ph == 0 && xflags == (XF_CON | XF_NOSTORE);
  const bool window = snap || (e->M.window && e->S.wbuf && (ph & PH_STEP2) && !(ph & (PH_NOINT | PH_PRE | PH_POST)) && !(xflags & ~(XF_FORCE | XF_DEFER | (wmode == 1 ? XF_PROF : 0))));
  if (window && !snap) ph |= PH_PRE;
  if (wmode && !window) { mjh_set_error("internal: window-chain launch mode on a launch that is not one"); return MJH_ERR_STATE; }
  if (wmode == 1) xflags |= XF_DEFER;
  if (wmode != 2) {
#define MJH_LAUNCH2(NR, DG, CX) do { if (e->H.has_hfield) HIPCHK(mjh_launch_step_hf(st, NR, DG, 0, n, (size_t)e->lds_bytes, e->dC, e->S, env0, nsteps, ph, xflags)); \
                                   else hipLaunchKernelGGL((mjh_step_kernel<NR, DG, CX>), dim3(n), dim3(64), (size_t)e->lds_bytes, st, e->dC, e->S, env0, nsteps, ph, xflags); } while (0)
#define MJH_LAUNCH(NR, DG) do { if (extra_instance(e->M) || e->S.xfrc_applied || e->report) MJH_LAUNCH2(NR, DG, true); else MJH_LAUNCH2(NR, DG, false); } while (0)
  const int nr = e->M.big ? 8 : (e->M.nv <= 16 ? 1 : (e->M.nv <= 32 ? 2 : 4));   // 8: many-body layout, running acceleration in LDS
  static const bool slim = !(getenv("MJH_WINDOW_SLIM") && atoi(getenv("MJH_WINDOW_SLIM")) == 0);
  if (window && slim) {
    // the assemble-only instance (WPRE): the step kernel without any sweep of its own — 116 - 119 VGPRs (allocated: 120) instead of 236, so that
    // its waves fit beside the lean window kernel's on a SIMD (376 + 120 <= 512 registers: tests/test_window_register_budget.py)
    const bool cx = extra_instance(e->M) || e->S.xfrc_applied || e->report;
    static const bool slim_lds = !(getenv("MJH_WINDOW_SLIM_LDS") && atoi(getenv("MJH_WINDOW_SLIM_LDS")) == 0);
    static const int wpad = getenv("MJH_WPRE_LDS_PAD") ? std::max(0, atoi(getenv("MJH_WPRE_LDS_PAD"))) : 0;      // (occupancy experiments: bytes of unused LDS per assemble-only workgroup)
    const size_t wlds = (size_t)((slim_lds && e->lds_bytes_pre > 0) ? e->lds_bytes_pre : e->lds_bytes) + (size_t)wpad;
    // (models of up to 64 contacts keep the base-row pool in LDS — instance 1 —, larger ones in the env's window slice — instance 2: derive_device_model)
#define MJH_LAUNCHW(NR, CX, GJ) do { if (e->H.has_hfield) HIPCHK(mjh_launch_step_hf(st, NR, true, GJ, n, wlds, e->dC, e->S, env0, nsteps, ph, xflags)); \
                                   else hipLaunchKernelGGL((mjh_step_kernel<NR, true, CX, GJ>), dim3(n), dim3(64), wlds, st, e->dC, e->S, env0, nsteps, ph, xflags); } while (0)
#define MJH_LAUNCHW2(NR, CX) do { if (e->M.patch) MJH_LAUNCHW(NR, CX, 1); else MJH_LAUNCHW(NR, CX, 2); } while (0)
    if (nr == 1) { if (cx) MJH_LAUNCHW2(1, true); else MJH_LAUNCHW2(1, false); } else { if (cx) MJH_LAUNCHW2(2, true); else MJH_LAUNCHW2(2, false); }
#undef MJH_LAUNCHW2
#undef MJH_LAUNCHW
  } else
  if (e->M.diagM) { if (nr == 1) MJH_LAUNCH(1, true); else if (nr == 2) MJH_LAUNCH(2, true); else if (nr == 4) MJH_LAUNCH(4, true); else MJH_LAUNCH(8, true); }
  else { if (nr == 1) MJH_LAUNCH(1, false); else if (nr == 2) MJH_LAUNCH(2, false); else if (nr == 4) MJH_LAUNCH(4, false); else MJH_LAUNCH(8, false); }
#undef MJH_LAUNCH2
#undef MJH_LAUNCH
  HIPCHK(hipGetLastError());
  }
  if (window && wmode != 1 && wmode != 3) {
    // LDS tier: windows beyond the register-resident ones, as many as leave four waves per CU (40 KB per wave)
    const int nl = tier_nl >= 0 ? tier_nl : window_tier(e);
    const size_t lds = (size_t)4 * nl * WN_XREC(e->M.win_nvt) * 16 * sizeof(float);
    // 24-dof models: a first section of wavefronts sweeps the envs with many rows in 32-row windows, two per wavefront (they scan the
    // same launch order and take the envs the assemble launch marked; almost all of them exit at once)
    const int n32 = (e->S.win32 && e->M.win_nvt == 24) ? (n + 1) / 2 : 0;
    const int wxf = (xflags & ~XF_DEFER) | ((ph & PH_STEP1) ? 0 : XF_SPLIT2) | (e->win_straight ? XF_WSTRAIGHT : 0);
    const int n64 = (e->S.win64 && e->M.win_nvt == 24 && e->S.win64 < 16 * e->M.win_maxw) ? n : 0;      // the 64-row section: one wavefront per env of the launch order, almost all of them exit at once
    HIPCHK(mjh_launch_window(st, e->M.win_nvt, n64 + (e->M.win_nvt == 24 ? n32 : 0) + (n + 3) / 4, lds, e->dC, e->S, env0, n, nl, wxf, n32, n64));
  }
  return MJH_OK;
}

static int launch(mjh_engine* e, int env0, int n, int nsteps, int ph, int xflags, int wmode = 0) { return launch_on(e, e->stream, env0, n, nsteps, ph, xflags, wmode); }

static int fork_cohorts(mjh_engine* e) {
  if (e->forked || e->ncohort <= 1) return MJH_OK;
  HIPCHK(hipEventRecord(e->ev_fork, e->stream));
  for (int g = 0; g < e->ncohort; g++) HIPCHK(hipStreamWaitEvent(e->cstream[g], e->ev_fork, 0));
  e->forked = true;
  return MJH_OK;
}
static int join_cohorts(mjh_engine* e) {
  if (!e->forked) return MJH_OK;
  for (int g = 0; g < e->ncohort; g++) {
    HIPCHK(hipEventRecord(e->ev_join[g], e->cstream[g]));
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join[g], 0));
  }
  e->forked = false;
  return MJH_OK;
}
static int set_cohorts(mjh_engine* e, int n) {
  n = std::max(1, std::min(n, MJH_MAX_COHORTS));
  int rc = join_cohorts(e);
  if (rc) return rc;
  if (n > 1) {
    if (!e->ev_fork) HIPCHK(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
    for (int g = 0; g < n; g++) {
      if (!e->cstream[g]) HIPCHK(hipStreamCreateWithFlags(&e->cstream[g], hipStreamNonBlocking));
      if (!e->ev_join[g]) HIPCHK(hipEventCreateWithFlags(&e->ev_join[g], hipEventDisableTiming));
    }
  }
  e->ncohort = n;
  return MJH_OK;
}

static int pair_cap(int t1, int t2) {
  if (t1 > t2) std::swap(t1, t2);
  if (t1 == MJH_GEOM_PLANE && t2 == MJH_GEOM_BOX) return 4;
  if (t1 == MJH_GEOM_PLANE && t2 == MJH_GEOM_CAPSULE) return 2;
  if (t1 == MJH_GEOM_PLANE && t2 == MJH_GEOM_CYLINDER) return 4;
  if (t1 == MJH_GEOM_PLANE && t2 == MJH_GEOM_MESH) return 4;
  if (t1 == MJH_GEOM_BOX && t2 == MJH_GEOM_BOX) return 8;
  if (t1 == MJH_GEOM_HFIELD) return MJH_HFIELD_MAXCON;       // (hfield-x: raw staging of the pair's first contacts in prism order)
  return 1;
}

// Host-only derivation of the device model: packed tables, derived topology tables, capacities and the LDS
// layout.  Needs no HIP device (mjh_query_lds_bytes uses it for capacity planning and in the CPU tests).
struct HostPack { DModel M{}; Lay L{}; DHField H{}; DWpre W{}; bool report = false; std::vector<int> I; std::vector<float> F; int o_controlled = 0, o_odom = 0, lds_bytes = 0, lds_bytes_pre = 0, lds_bytes_wpre = 0; long long gstride = 0; };      // lds_bytes_pre: an assemble-only launch's extent in the fused layout's own offsets; lds_bytes_wpre: what that launch allocates
// Gauss-Seidel order of engines created afterwards (mjhip.h): 1 = mj_solPGS's own row order
#define MJH_WINDOW_MAXCON 128    // contact capacity up to which a small free-body model steps through the window chain
static int g_window_solver = getenv("MJH_WINDOW") ? (atoi(getenv("MJH_WINDOW")) != 0) : 1;
extern "C" void mjh_set_window_solver(int on) { g_window_solver = on ? 1 : 0; }
static int g_pgs_row_order = 1;
// Contact report of engines created afterwards (mjhip.h): the step kernel leaves the contacts with their solver forces and cfrc_ext per env.
// Such an engine lays its model out as it would a model with a force sensor (the report reads the position stage, the contact records and the
// block forces after the solve): no diagonal-M form, no patch sweep, no window chain, one fused launch per step in the many-body layout
static int g_contact_report = getenv("MJH_CONTACT_REPORT") ? (atoi(getenv("MJH_CONTACT_REPORT")) != 0) : 0;
extern "C" void mjh_set_contact_report(int on) { g_contact_report = on ? 1 : 0; }
extern "C" void mjh_set_pgs_row_order(int mode) { g_pgs_row_order = mode < 0 || mode > 2 ? 1 : mode; }
static void derive_device_model(const mjh_model* m, HostPack& hp, bool force_big = false, bool allow_patch = true) {
  DModel& M = hp.M; std::vector<int>& I = hp.I; std::vector<float>& F = hp.F;
  const bool report = g_contact_report != 0;
  hp.report = report;
  // ---- derived integer tables
  const int nb = m->nbody, nv = m->nv, nj = m->njnt, ng = m->ngeom;
  std::vector<int> subtreesize(nb, 1), lastdof(nb, -1), stageadr(m->npair, 0), fl_dof, gc_body, controlled(std::max(nv, 1), 0), odom(10, -1);
  odom[9] = 0;
  for (int b = nb - 1; b > 0; b--) subtreesize[m->body_parentid[b]] += subtreesize[b];
  for (int b = 1; b < nb; b++) lastdof[b] = m->body_dofnum[b] ? m->body_dofadr[b] + m->body_dofnum[b] - 1 : lastdof[m->body_parentid[b]];
  int nstage = 0, maxlevel = 0, rowW = 1;
  for (int b = 0; b < nb; b++) maxlevel = std::max(maxlevel, m->body_level[b]);
  auto treenum = [&](int b) { int t = m->body_treeid[b]; return t >= 0 ? m->tree_dofnum[t] : 0; };
  for (int i = 0; i < m->npair; i++) {
    int g1 = m->pair_geom1[i], g2 = m->pair_geom2[i];
    stageadr[i] = nstage; nstage += pair_cap(m->geom_type[g1], m->geom_type[g2]);
    int b1 = m->geom_bodyid[g1], b2 = m->geom_bodyid[g2];
    int w = treenum(b1) + ((m->body_treeid[b1] != m->body_treeid[b2]) ? treenum(b2) : 0);
    rowW = std::max(rowW, w);
  }
  for (int t = 0; t < m->ntree; t++) rowW = std::max(rowW, m->tree_dofnum[t]);
  int neqrow = 0; bool has_weld = false;
  for (int q = 0; q < m->neq; q++) {
    if (m->eq_type[q] != MJH_EQ_JOINT) {      // connect / weld between bodies: 3 / 6 single-row blocks over the bodies' trees
      has_weld = true; neqrow += m->eq_type[q] == MJH_EQ_WELD ? 6 : 3;
      rowW = std::max(rowW, treenum(m->eq_obj1id[q]) + ((m->body_treeid[m->eq_obj1id[q]] != m->body_treeid[m->eq_obj2id[q]]) ? treenum(m->eq_obj2id[q]) : 0));
      continue;
    }
    neqrow++;
    int j1 = m->eq_obj1id[q], j2 = m->eq_obj2id[q];
    int t1 = m->dof_treeid[m->jnt_dofadr[j1]], w = m->tree_dofnum[t1];
    if (j2 >= 0) { int t2 = m->dof_treeid[m->jnt_dofadr[j2]]; if (t2 != t1) w += m->tree_dofnum[t2]; }
    rowW = std::max(rowW, w);
  }
  rowW = ((rowW + 3) / 4) * 4;
  // every tree a single free body about its own COM with principal axes = body axes  =>  M is diagonal
  bool diagM = m->ntree > 0 && m->neq == 0 && m->nsensor == 0 && m->nmocap == 0 && !report;   // (also implies: no limit / equality rows, every block is a contact)
  for (int t = 0; t < m->ntree && diagM; t++) {
    const int b = m->tree_bodyid[t];
    diagM = m->tree_dofnum[t] == 6 && m->body_jntnum[b] == 1 && m->jnt_type[m->body_jntadr[b]] == MJH_JNT_FREE && subtreesize[b] == 1 &&
            m->body_ipos[3*b] == 0 && m->body_ipos[3*b+1] == 0 && m->body_ipos[3*b+2] == 0 && m->body_iquat[4*b] == 1;
  }
  bool has_damping = false, has_limits = false;
  for (int d = 0; d < nv; d++) { if (m->dof_frictionloss[d] > 0) { fl_dof.push_back(d); diagM = false; } if (m->dof_damping[d] > 0) has_damping = true; }
  for (int j = 0; j < nj; j++) if (m->jnt_limited[j]) has_limits = true;
  for (int b = 1; b < nb; b++) if (m->body_gravcomp[b] != 0) gc_body.push_back(b);

  // ---- pack tables
  auto addI = [&](const int* p, size_t n) { int o = (int)I.size(); I.insert(I.end(), p, p + n); while (I.size() % 4) I.push_back(0); return o; };
  auto addF = [&](const double* p, size_t n) { int o = (int)F.size(); for (size_t i = 0; i < n; i++) F.push_back((float)p[i]); while (F.size() % 4) F.push_back(0); return o; };
#define PI(name, n) M.o_##name = addI(m->name, (size_t)(n))
#define PF(name, n) M.o_##name = addF(m->name, (size_t)(n))
  PI(body_parentid, nb); PI(body_rootid, nb); PI(body_jntadr, nb); PI(body_jntnum, nb); PI(body_dofadr, nb); PI(body_dofnum, nb);
  PI(body_level, nb); M.o_body_subtreesize = addI(subtreesize.data(), nb); PI(body_treeid, nb); M.o_body_lastdof = addI(lastdof.data(), nb);
  PI(jnt_type, nj); PI(jnt_qposadr, nj); PI(jnt_dofadr, nj); PI(jnt_bodyid, nj); PI(jnt_limited, nj);
  PI(dof_bodyid, nv); PI(dof_jntid, nv); PI(dof_parentid, nv); PI(dof_Madr, nv); PI(dof_treeid, nv);
  PI(tree_dofadr, m->ntree); PI(tree_dofnum, m->ntree);
  PI(geom_type, ng); PI(geom_bodyid, ng); PI(geom_condim, ng);
  PI(pair_geom1, m->npair); PI(pair_geom2, m->npair); M.o_pair_stageadr = addI(stageadr.data(), m->npair);
  PI(eq_obj1id, m->neq); PI(eq_obj2id, m->neq); PI(eq_active, m->neq);
  M.o_fl_dof = addI(fl_dof.data(), fl_dof.size()); M.o_gc_body = addI(gc_body.data(), gc_body.size());
  M.o_controlled = hp.o_controlled = addI(controlled.data(), controlled.size());
  M.o_odom = hp.o_odom = addI(odom.data(), odom.size());
  PF(body_pos, 3*nb); PF(body_quat, 4*nb); PF(body_ipos, 3*nb); PF(body_iquat, 4*nb); PF(body_mass, nb); PF(body_inertia, 3*nb);
  PF(body_gravcomp, nb); PF(body_invweight0, 2*nb);
  PF(jnt_pos, 3*nj); PF(jnt_axis, 3*nj); PF(jnt_stiffness, nj); PF(jnt_range, 2*nj); PF(jnt_margin, nj); PF(jnt_solref, 2*nj); PF(jnt_solimp, 5*nj);
  PF(qpos0, m->nq); PF(qpos_spring, m->nq);
  PF(dof_armature, nv); PF(dof_damping, nv); PF(dof_frictionloss, nv); PF(dof_invweight0, nv); PF(dof_solref, 2*nv); PF(dof_solimp, 5*nv);
  PF(geom_pos, 3*ng); PF(geom_quat, 4*ng); PF(geom_size, 3*ng); PF(geom_rbound, ng); PF(geom_friction, 3*ng); PF(geom_solmix, ng);
  PF(geom_solref, 2*ng); PF(geom_solimp, 5*ng); PF(geom_margin, ng); PF(geom_gap, ng);
  PF(eq_data, 11*m->neq); PF(eq_solref, 2*m->neq); PF(eq_solimp, 5*m->neq);
  PI(geom_dataid, ng); PI(mesh_vertadr, m->nmesh); PI(mesh_vertnum, m->nmesh); PF(mesh_vert, 3 * (size_t)m->nmeshvert);
  PI(eq_type, m->neq);
  if (m->nsite > 0) { PI(site_bodyid, m->nsite); PF(site_pos, 3 * (size_t)m->nsite); PF(site_quat, 4 * (size_t)m->nsite); }
  if (m->nsensor > 0) { PI(sensor_type, m->nsensor); PI(sensor_objid, m->nsensor); }
  {
    std::vector<int> mocapid(nb, -1);
    if (m->body_mocapid) for (int b = 0; b < nb; b++) mocapid[b] = m->body_mocapid[b];
    M.o_body_mocapid = addI(mocapid.data(), nb);
  }
  M.nsite = m->nsite; M.nsensor = m->nsensor; M.nmocap = m->nmocap; M.has_weld = has_weld ? 1 : 0;
  {   // height fields: packed behind every other table (models without hfield pairs keep their tables exactly)
    DHField& H = hp.H;
    H.has_hfield = 0;
    for (int i = 0; i < m->npair; i++) if (m->geom_type[m->pair_geom1[i]] == MJH_GEOM_HFIELD) H.has_hfield = 1;
    if (H.has_hfield) {
      H.o_hfield_nrow = addI(m->hfield_nrow, m->nhfield); H.o_hfield_ncol = addI(m->hfield_ncol, m->nhfield); H.o_hfield_adr = addI(m->hfield_adr, m->nhfield);
      H.o_hfield_size = addF(m->hfield_size, 4 * (size_t)m->nhfield); H.o_hfield_data = addF(m->hfield_data, (size_t)m->nhfielddata);
    }
  }
  // groups of up to 16 mutually independent blocks (four waves x four 16-lane rows in mjh_solve_kernel) when a tree bitmask fits
  // one 64-bit word and every block fits a 16-lane row; else 4 (same rule as the oracle's m_group_max)
  M.group_max = m->ntree <= 64 ? 16 : 4;
  for (int t = 0; t < m->ntree; t++) if (m->tree_dofnum[t] > 8) M.group_max = 4;
#undef PI
#undef PF
  M.nq = m->nq; M.nv = nv; M.nbody = nb; M.njnt = nj; M.ngeom = ng; M.neq = m->neq; M.npair = m->npair; M.nM = m->nM; M.ntree = m->ntree;
  M.maxcon = std::max(m->maxcon, 1); M.maxefc = std::max(m->maxefc, 1);
  // per-env state record: the rows a step reads (qpos, qvel, qacc_warmstart, ddq, dq) lie back to back in one record per
  // env, padded to whole 128-byte lines (S24: 28 + 4 x 24 floats = 496 B -> 4 lines; as five separately padded rows it
  // was 5 lines), and every per-env array uses the record stride (the kernel knows only (pointer, stride) pairs)
  M.nqp = M.nvp = pad32(m->nq + 4 * std::max(nv, 1));
  M.maxlevel = maxlevel; M.nfl = (int)fl_dof.size(); M.ngc = (int)gc_body.size(); M.rowW = rowW; M.nstage = nstage;
  M.has_damping = has_damping; M.has_limits = has_limits; M.diagM = diagM;
  M.has_dim4 = 0;
  for (int g = 0; g < ng; g++) if (m->geom_condim[g] == 4) M.has_dim4 = 1;
  M.has_convex = 0;   // some pair needs the generic convex narrow phase (cylinder-x, capsule-box, ellipsoid-x)
  for (int i = 0; i < m->npair; i++) {
    const int t1 = m->geom_type[m->pair_geom1[i]], t2 = m->geom_type[m->pair_geom2[i]];
    if (t2 == MJH_GEOM_MESH) M.has_convex = 1;
    if (t1 != MJH_GEOM_PLANE && (t1 == MJH_GEOM_ELLIPSOID || t2 == MJH_GEOM_ELLIPSOID || t1 == MJH_GEOM_CYLINDER || t2 == MJH_GEOM_CYLINDER ||
                                 t2 == MJH_GEOM_MESH || (t1 == MJH_GEOM_CAPSULE && t2 == MJH_GEOM_BOX))) M.has_convex = 1;
  }
  {
    // a limited joint can have both sides active only if its margins overlap (range narrower than 2 margins)
    int nlim = 0; for (int j = 0; j < nj; j++) if (m->jnt_limited[j]) nlim += (m->jnt_range[2*j+1] - m->jnt_range[2*j] <= 2 * m->jnt_margin[j]) ? 2 : 1;
    const int nfix = neqrow + (int)fl_dof.size() + nlim;
    M.maxblk = nfix + M.maxcon; M.maxbrow = nfix + 4 * M.maxcon;
  }
  M.iterations = m->opt.iterations; M.disableflags = m->opt.disableflags;
  M.timestep = (float)m->opt.timestep; M.timestep_d = m->opt.timestep; for (int k = 0; k < 3; k++) M.gravity[k] = (float)m->opt.gravity[k];
  M.tolerance = (float)m->opt.tolerance; M.impratio = (float)m->opt.impratio; M.meaninertia = (float)m->meaninertia;
  M.noslip_iterations = m->opt.noslip_iterations; M.noslip_tolerance = (float)m->opt.noslip_tolerance;
  // ---- LDS layout (float offsets, 16-byte aligned)
  {
    Lay& L = hp.L; int off = 0; long long goff = 0;
    auto put = [&](int n) { int o = off; off += ((std::max(n, 1) + 3) / 4) * 4; return o; };
    // many-body models (nv > 64, NROW = 8 kernels): the contact / block / Jacobian pools go to a per-env slice of global
    // memory (negative offsets), only the per-body / per-dof arrays stay in LDS
    const bool big = force_big || nv > 64;
    M.big = big;
    // models with sensors read the position-stage arrays, the contact records and the velocity-stage vectors again AFTER the
    // solver (mj_sensorAcc): nothing of those is aliased then
    // ... and so does the contact report
    const bool keep = m->nsensor > 0 || report;
    auto gput = [&](long long n) { long long o = goff; goff += ((std::max<long long>(n, 1) + 3) / 4) * 4; return (int)(-1 - o); };
    const int nblkcap = std::max(M.maxblk, 1);   // exact: the block builder never creates more than maxblk blocks
    // J / B pools: one row per non-contact block (equality, friction loss, limits), four interleaved rows per contact
    long long jsz = std::max<long long>((long long)(M.maxblk - M.maxcon) * rowW + (long long)M.maxcon * rowW * 4, 4);
    const long long need = (long long)nstage * RAW_STRIDE;            // raw-contact staging aliases J (+B)
    if ((diagM ? 1 : 2) * jsz < need) jsz = diagM ? need : (need + 1) / 2;
    // contact-patch sweep (patch_pgs.h): free bodies only, no noslip pass, pools in LDS, at most 64 contacts (the patch builder
    // keeps one contact per lane).  Same rule as the oracle's patch order (oracle/mjh_oracle.c: m_patch_order).
    // Gauss-Seidel order (mjh_set_pgs_row_order).  1 (default): mj_solPGS's own constraint-row order, blocks without a common kinematic
    // tree side by side under a precedence-preserving list schedule (bit-identical to the sequential sweep: 2).  0: the legacy orders
    // that reorder conflicting blocks (patch / pair / group first fit) — except for the models whose sweeps are sequential in either
    // layout anyway (more than 32 dofs and a kinematic tree of more than 16: articulated robots), which always run row order;
    // same rules as the oracle's (oracle/mjh_oracle.c: m_row_order)
    M.pgs_row_order = g_pgs_row_order;
    if (!M.pgs_row_order && nv > 32) for (int t = 0; t < m->ntree; t++) if (m->tree_dofnum[t] > 16) M.pgs_row_order = 1;
    const bool small_free = allow_patch && diagM && !big && nv <= 32 && M.noslip_iterations == 0 && !keep;
    const bool patch = small_free && M.maxcon <= 64;
    M.patch = patch ? 1 : 0;
    // window sweep (window_pgs.h): mjh_step of a small free-body model in row order = assemble launch + mjh_window_kernel (MJH_WINDOW=0 /
    // mjh_set_window_solver(0): the fused kernel's sweep instead — same order, same iterates up to fp32 rounding).  The window chain
    // has no tie to one contact per lane: models of this class with a contact capacity of 65 .. MJH_WINDOW_MAXCON keep the LDS-resident
    // layout WITHOUT the patch sweep (the fused kernel's dual-block sweep, list-scheduled in the same row order, serves the launches
    // that are not whole steps) and step through the window chain (mj_collision itself has no cap: mj_main.cpp:83)
    M.window = (small_free && M.maxcon <= MJH_WINDOW_MAXCON && M.pgs_row_order != 0 && g_window_solver && nv <= 32 && m->njnt <= 16 && m->nq <= 40) ? 1 : 0;
    M.win_nvt = nv <= 24 ? 24 : 32;
    M.win_maxw = std::max(1, std::min(WN_MAXW, (M.maxefc + 15) / 16));
    // (tests: MJH_WINDOW_MAXW lowers a model's window capacity below its row capacity, so that the hand-over's own capacity rule — whole blocks
    //  dropped behind the last one that fits, window_emit — can be met with a few dozen rows instead of more than 16 WN_MAXW = 384)
    if (const char* v = getenv("MJH_WINDOW_MAXW")) M.win_maxw = std::max(1, std::min(M.win_maxw, atoi(v)));
    L.qpos = put(m->nq);
    L.qvel = put(nv); L.qvref = put(nv); L.ws = put(nv); L.qacc = put(nv); L.smooth = put(nv); L.asmooth = put(nv); L.passive = put(nv);
    L.bias = put(nv); L.applied = put(nv); L.tmpv = put(nv); L.tmpv2 = put(nv);
    if (patch) {   // what the sweep still needs sits in front of the span the patch pool takes over
      L.qM = put(m->nM); L.qLD = L.qM; L.qLDinv = put(nv); L.dofpar = 0; L.dofMadr = 0; L.anc = 0;
      L.p_gsize = put(3*ng); L.p_rbound = put(ng); L.p_mass = put(nb); L.p_inertia = put(3*nb);
      L.zero = put(PP_ZERO);     // (a lane outside a patch reads a whole row record of zeros)
    }
    // K1: frames, composite inertias, joint anchors/axes and geom poses are dead once the position stage, CRBA and the
    // collision stage are done; the solver's per-base scratch vectors (bv, phi: first used by the velocity stage) reuse them
    const int k1 = off;
    // free-body models (diagM) form neither composite / spatial inertias nor motion axes nor the spatial velocity-stage vectors
    // (closed forms in step_kernel.h): those arrays all alias one unused slot
    const int unused = diagM ? put(4) : 0;
    L.xpos = put(3*nb); L.xquat = put(4*nb); L.xmat = put(9*nb); L.ximat = put(9*nb); L.crb = diagM ? unused : put(10*nb);
    L.xanchor = put(3*nj); L.xaxis = put(3*nj); L.gpos = put(3*ng); L.gmat = put(9*ng);
    const int k1_size = off - k1;
    M.k1_floats = k1_size;
    M.scratch_off = (big && keep) ? put(k1_size) : k1;
    L.xipos = put(3*nb); L.com = put(3*nb); L.cinert = diagM ? unused : put(10*nb); L.cdof = diagM ? unused : put(6*nv);
    const int k2_size = off - k1;   // ... and all of these are dead when the solver sweeps run: the X extension of condim-4 models
    if (!patch) {
      // diagonal M: no factor storage; many-body layout: the factor is built in M's place (M itself stays in the env's scratch slice)
      L.qM = put(m->nM); L.qLD = (diagM || big) ? L.qM : put(m->nM); L.qLDinv = put(nv);
      if (diagM) { L.dofpar = 0; L.dofMadr = 0; L.anc = 0; }   // free-body models read the shared chain-walk tables (step_kernel.h)
      else { L.dofpar = put(nv); L.dofMadr = put(nv); L.anc = put(m->nM); }
      // (models without a collision pair never read the per-env geom sizes / bounding radii: their copies land in the geom poses' span instead of
      //  taking their own — C3, four arms per wavefront: 20816 -> 20336 B, 17 -> 16 LDS granules, 7 -> 8 workgroups per CU = all 2048 resident)
      const bool nopairs = m->npair == 0;
      L.p_gsize = nopairs ? L.gpos : put(3*ng); L.p_rbound = nopairs ? L.gmat : put(ng); L.p_mass = put(nb); L.p_inertia = put(3*nb);
    }
    {  // the contact records die once the blocks are built; the velocity-stage spatial vectors reuse their space
      const int a4 = [](int n) { return ((std::max(n, 1) + 3) / 4) * 4; }(6*nb);
      const int velsz = diagM ? 4 : 4 * a4 + ((6*nv + 3) / 4) * 4;
      int vel;
      // (many-body layout: they reuse the position-stage arrays instead, which are dead when the velocity stage starts)
      if (big) { L.con = gput((long long)M.maxcon * CON_STRIDE); L.blkq = gput((long long)nblkcap * BLKQ_STRIDE); vel = (!keep && !diagM && velsz <= k1_size) ? k1 : put(velsz); }
      else if (keep) { L.con = put(M.maxcon * CON_STRIDE); L.blkq = put(nblkcap * BLKQ_STRIDE); vel = put(velsz); }
      else {
        // (and, once those are dead too, the per-block solver matrices A_c / Q, built when the solver starts)
        L.con = put(std::max(std::max(M.maxcon * CON_STRIDE, velsz), nblkcap * BLKQ_STRIDE));
        L.blkq = L.con; vel = L.con;
      }
      if (diagM) { L.cvel = unused; L.cacc = unused; L.cfrc = unused; L.cfrcsub = unused; L.cdofdot = unused; }
      else { L.cvel = vel; L.cacc = vel + a4; L.cfrc = vel + 2*a4; L.cfrcsub = vel + 3*a4; L.cdofdot = vel + 4*a4; }
    }
    const int extsz = (M.has_dim4 && !patch) ? nblkcap * SOLX_N : 0;   // (the patch sweep does not use the condim-4 extension)
    int jpre = 0;      // LDS-resident layouts: the end of blkf — where a patch model's assemble-only instance puts its base rows (below)
    if (big) {
      L.blki = gput((long long)nblkcap * BLKI_STRIDE); L.blkf = gput((long long)nblkcap * BLKF_STRIDE);
      L.bv = gput((long long)nblkcap * 4); L.phi = gput((long long)nblkcap * 4); L.sched = gput((long long)nblkcap * 2); L.order = gput(nblkcap);
      L.ext = gput(extsz); L.J = gput(jsz); L.B = diagM ? L.J : gput(jsz);
    } else {
      L.blki = put(nblkcap * BLKI_STRIDE); L.blkf = put(nblkcap * BLKF_STRIDE);
      // window-only models (65 .. 128 contacts): their assemble-only launch (WPRE instance 2) builds no block schedule and no condim-4
      // extension — both belong to the fused kernel's sweep — and keeps the per-base scratch vectors bv / phi (first written by the
      // velocity stage) in the contact records, which are dead by then (step_kernel.h; the fused instance cannot: its A_c / Q matrices
      // take that span while phi is live).  Its LDS ends in front of all of them: S24D at capacity 96 25.3 -> 16.9 KB, 6 -> 9
      // environments per CU (5.30 -> 5.6 M env-steps/s, bitwise).  MJH_WPRE_SLIM2=0: the former extent
      static const bool slim2 = !(getenv("MJH_WPRE_SLIM2") && atoi(getenv("MJH_WPRE_SLIM2")) == 0);
      const bool wonly = M.window && !patch && slim2 && 8 * nblkcap <= M.maxcon * CON_STRIDE;
      if (wonly) hp.lds_bytes_pre = off * (int)sizeof(float);
      jpre = off;
      if (2 * nblkcap * 4 <= k1_size && !keep) { L.bv = k1; L.phi = k1 + nblkcap * 4; }
      else { L.bv = put(nblkcap * 4); L.phi = put(nblkcap * 4); }
      L.sched = put(nblkcap * 2);
      // the dual-block sweep (nv <= 32) reads the pair schedule only; `order` is then just scratch of the schedule builder
      L.order = (nv <= 32 && nblkcap <= k1_size && !keep) ? L.bv : put(nblkcap);
      L.ext = (extsz <= k2_size && !keep) ? k1 : put(extsz);
      // (window models beyond 64 contacts: the base-row pool comes last, their assemble-only launch keeps it in global memory and allocates the LDS in front of it)
      if (!wonly) hp.lds_bytes_pre = off * (int)sizeof(float);
      L.J = put((int)jsz); L.B = diagM ? L.J : put((int)jsz);
    }
    M.win_jsz = (int)jsz;
    if (!(M.window && !big && !patch)) hp.lds_bytes_pre = off * (int)sizeof(float);    // everything but the patch pool's own tail: what an assemble-only launch (window chain) touches
    // Patch models on the window chain (S24): their assemble-only launch (WPRE instance 1) builds no pair schedule either and keeps bv / phi in
    // the contact records like instance 2 (8 nblkcap <= maxcon CON_STRIDE: a patch model has no block but its contacts), so its base-row pool
    // — in LDS still — starts where the fused kernel's layout has bv: S24 18192 -> 16592 B, 15 -> 13 granules of 1280 B.  Beside three window
    // wavefronts (15 granules each) a CU then holds six of these workgroups instead of five: all 1365 of a cohort of the headline start at
    // once, where about 30 started 5 - 25 us late and set the launch's end (56 -> 40 us, S24 14.95 -> 15.70 M env-steps/s, bitwise:
    // profiles/assemble_round_summary.md).  Only W and this extent change: every offset in L, and with them every other instance, stay as
    // they are.  MJH_WPRE_SLIM3=0: the former extent.
    static const bool slim3 = !(getenv("MJH_WPRE_SLIM3") && atoi(getenv("MJH_WPRE_SLIM3")) == 0);
    // (lds_bytes_pre — mjh_query_lds_bytes_assemble — stays the extent in the fused layout's offsets, an upper bound for these models; what the
    //  launch allocates is lds_bytes_wpre, reported by mjh_debug_lds_layout)
    int wpre_floats = 0;
    if (slim3 && M.window && patch && !big && 8 * nblkcap <= M.maxcon * CON_STRIDE) { hp.W.slim = 1; hp.W.J = jpre; wpre_floats = jpre + (int)jsz; }
    if (patch) {
      // the pool: per patch of nr4 rows (a multiple of 4, at most 16) a record per row (20 floats between two bodies, 12 on one
      // body) + 16 floats per 4x4 tile of the lower triangle of AR: 16 .. 30 floats per row.  It takes the span of everything that
      // is dead by then and no more (S24: 3948 floats; a 20 000-step soak of 4096 envs never fills it); patches beyond it are
      // dropped with the capacity flag, like contacts beyond maxcon
      // The two small tables the sweep reads next to the pool (one descriptor per patch, one per schedule slot) sit in front
      // of it: that space (position-stage arrays, contact records) is dead when they are written, unlike the span's tail.
      M.pdesc = k1; M.pslot = k1 + ((M.maxcon + 3) / 4) * 4; M.pool = M.pslot + 4 * M.maxcon;
      M.pool_floats = std::max(off - M.pool, (33 * M.maxefc) / 2);   // (at least what the span was before free-body models dropped their spatial arrays: a 20 000-step soak never filled that)
      if (const char* cap = getenv("MJH_PATCH_POOL_FLOATS")) M.pool_floats = std::max(512, std::min(M.pool_floats, atoi(cap)));   // (tests: the drop rule)
      off = std::max(off, M.pool + M.pool_floats);
      if (!getenv("MJH_PATCH_POOL_FLOATS")) {
        // LDS is handed out in 1280-byte granules and a CU holds floor(128 / granules) workgroups: the pool takes what is left of
        // the last granule that costs no workgroup (S24: 15 -> 16 granules at 8 per CU, +12 % pool)
        const int gran = (off * 4 + 1279) / 1280, wg = 128 / std::max(gran, 1);
        if (wg >= 1) { const int room = std::min((128 / wg) * 320, 16384); if (room > off) { M.pool_floats += room - off; off = room; } }
      }
    } else L.zero = put(4);
    L.site = m->nsite > 0 ? put(12 * m->nsite) : 0;        // world frame of every site: pos(3) + rotation(9)
    L.fext = (m->nsensor > 0 || report) ? put(6 * nb) : 0;   // external spatial force per body (mj_rnePostConstraint; cfrc_ext of the contact report)
    // (the site frames / external forces sit behind the patch pool: an assemble-only launch of a model that has them gets the whole layout)
    if (m->nsite > 0 || m->nsensor > 0 || report) { hp.lds_bytes_pre = off * (int)sizeof(float); wpre_floats = 0; }
    hp.lds_bytes_wpre = wpre_floats ? wpre_floats * (int)sizeof(float) : hp.lds_bytes_pre;
    if (big) {   // hand-over vectors of the three-launch step (non-negative offsets into the scratch slice)
      auto graw = [&](int n) { long long o = goff; goff += ((std::max(n, 1) + 3) / 4) * 4; return (int)o; };
      L.g_a0 = graw(nv); L.g_minv = graw(nv); L.g_qvel = graw(nv); L.g_smooth = graw(nv); L.g_qacc = graw(nv); L.g_meta = graw(8); L.g_qM = graw(m->nM);
      // dense row-space solver (dense_pgs.h): articulated models (M not diagonal) without noslip sweeps, at most 128 dofs; an
      // env takes it in the steps in which it has at most dense_cap rows.  MJH_DENSE=0 keeps the block solver everywhere.
      const bool dense_on = !(getenv("MJH_DENSE") && atoi(getenv("MJH_DENSE")) == 0);
      M.dense = (dense_on && !diagM && M.noslip_iterations == 0 && nv <= 128 && nv >= 1) ? 1 : 0;
      M.dense_cap = std::min(256, ((std::max(M.maxefc, 1) + 63) / 64) * 64); M.dense_nvs = ((nv + 15) / 16) * 16;
      if (const char* dc = getenv("MJH_DENSE_CAP")) M.dense_cap = std::max(64, std::min(M.dense_cap, (atoi(dc) / 64) * 64));   // (tests: envs beyond the capacity keep the block solver)
      M.dense_min_iter = getenv("MJH_DENSE_MIN_ITER") ? std::max(0, atoi(getenv("MJH_DENSE_MIN_ITER"))) : 32;
      L.g_dense = 0; L.g_qLD = 0; L.g_anc = 0;
      if (M.dense) { L.g_qLD = graw(m->nM); L.g_anc = graw(m->nM); }
      if (M.dense) { long long o = goff; goff += (long long)M.dense_cap * M.dense_cap + (long long)M.dense_cap * M.dense_nvs + 6LL * M.dense_cap; L.g_dense = (int)o; }
    }
    hp.gstride = goff;
    if (const char* pad = getenv("MJH_LDS_PAD")) off += std::max(0, atoi(pad));   // (occupancy experiments: floats of unused LDS per env)
    L.total = off;
    hp.lds_bytes = off * (int)sizeof(float);
  }
}

// Layout choice.  The LDS-resident layout wins for small free-body scenes (S24: 4.7 M env-steps/s against 1.6 M), the
// many-body layout (pools in global memory, three-launch step) wins as soon as the LDS-resident working set leaves only a
// few environments per CU (pr2 / tiago / hsrb4s / ridgeback_panda: 1.6x - 5x); a working set beyond one CU's LDS has no choice.
//   policy 0 (default): many-body layout above MJH_LDS_RESIDENT_MAX bytes;  1: LDS-resident whenever it fits;  2: many-body whenever possible
#define MJH_LDS_RESIDENT_MAX (24 * 1024)
// steps between renewals of a cohort's launch order.  The sort is one workgroup on the cohort's stream in front of a step: 6 us on an idle
// chip, 74 us (S24) to 200 us (C2) beside the other cohorts' resident waves; an env's cost drifts slowly.  8 / 16 / 32 / 64 steps: S24
// 11.29 / 11.46 / 11.52 / 11.40 M, C4 1.41 / 1.43 / 1.45 / 1.39 M, C2 0.541 / 0.545 / 0.546 / 0.544 M env-steps/s (tools/r04_order_every.sh)
#define MJH_ORDER_EVERY 32
// ... 16 for the window models whose envs reach the 64-row form's row counts (S24D: the slowest wavefront is a function of which envs share it,
// and the piles' row counts drift faster than the sweep counts of S24): 8 / 16 / 32 / 64 steps S24D 5.92 / 5.91 / 5.84 / 5.73 M, S24 13.60 /
// 13.75 / 13.82 / 13.75 M (round 6, tools/r06_knobs.sh).  Results do not depend on the launch order (bitwise: tests).
static int order_every_of(const mjh_engine* e);
static int g_layout_policy = 0;
extern "C" void mjh_set_layout_policy(int policy) { g_layout_policy = policy < 0 || policy > 2 ? 0 : policy; }
static int order_every_of(const mjh_engine* e) {
  static const int env = getenv("MJH_ORDER_EVERY") ? std::max(1, atoi(getenv("MJH_ORDER_EVERY"))) : 0;
  return env ? env : ((e->M.window && e->M.win_maxw > 16) ? 16 : MJH_ORDER_EVERY);
}
static void derive_fitting(const mjh_model* m, HostPack& hp) {
  derive_device_model(m, hp);
  int policy = g_layout_policy;
  if (const char* fb = getenv("MJH_FORCE_BIG")) policy = atoi(fb) ? 2 : 1;
  const int limit = policy == 1 ? 160 * 1024 : (policy == 2 ? 0 : MJH_LDS_RESIDENT_MAX);
  // (models on the contact-patch sweep stay LDS-resident under the default policy: their visiting order is the patch order,
  //  which the many-body layout does not have; mjh_solver_order() tells which one an engine runs)
  if ((hp.M.patch || hp.M.window) && policy == 0 && hp.lds_bytes <= 64 * 1024) return;
  // The patch sweep packs two LDS byte addresses into one 32-bit word (patch_pgs.h: laddr(x) | laddr(y) << 16), which holds
  // only while the workgroup's LDS stays within 64 KiB.  A patch model that would stay LDS-resident beyond that (policy 1 /
  // MJH_FORCE_BIG=0 with a large user-set maxefc) is re-derived WITHOUT the patch sweep (pair order, mjh_solver_order() = 0).
  if (hp.M.patch && hp.lds_bytes > 64 * 1024 && hp.lds_bytes <= limit) { HostPack np; derive_device_model(m, np, false, false); hp = np; }
  if ((hp.lds_bytes > 160 * 1024 || hp.lds_bytes > limit) && !hp.M.big && hp.M.rowW <= 64) { HostPack big; derive_device_model(m, big, true); hp = big; }
}

extern "C" int mjh_query_lds_bytes(const mjh_model* m) {
  if (!m) return MJH_ERR_ARG;
  HostPack hp; derive_fitting(m, hp);
  return hp.lds_bytes;
}
// the LDS layout of a model as text: "name offset" per array in float units (negative: the env's global slice), then the totals —
// capacity planning (which array costs a granule: tools/lds_layout.py).  Returns the number of bytes written (without the terminator)
extern "C" int mjh_debug_lds_layout(const mjh_model* m, char* out, int cap) {
  if (!m || !out || cap <= 0) return MJH_ERR_ARG;
  HostPack hp; derive_fitting(m, hp);
  std::string t;
#define X(n) t += std::string(#n) + " " + std::to_string(hp.L.n) + "\n";
  MJH_LDS_ARRAYS(X)
#undef X
  t += "total " + std::to_string(hp.L.total) + "\nlds_bytes " + std::to_string(hp.lds_bytes) + "\nlds_bytes_pre " + std::to_string(hp.lds_bytes_pre) +
       "\nk1_floats " + std::to_string(hp.M.k1_floats) + "\nmaxcon " + std::to_string(hp.M.maxcon) + "\nmaxblk " + std::to_string(hp.M.maxblk) +
       "\nrowW " + std::to_string(hp.M.rowW) + "\nnstage " + std::to_string(hp.M.nstage) + "\nbig " + std::to_string((int)hp.M.big) +
       "\nlds_bytes_wpre " + std::to_string(hp.M.window ? hp.lds_bytes_wpre : 0) + "\n";      // what the window chain's assemble-only launch allocates (0: the model does not take it)
  const int n = std::min((int)t.size(), cap - 1);
  std::memcpy(out, t.data(), (size_t)n); out[n] = 0;
  return n;
}
extern "C" int mjh_query_lds_bytes_assemble(const mjh_model* m) {   // ... of the assemble-only instance of the window chain (0: the model does not take it)
  if (!m) return MJH_ERR_ARG;
  HostPack hp; derive_fitting(m, hp);
  return hp.M.window ? hp.lds_bytes_pre : 0;
}

extern "C" int mjh_create(const mjh_model* m, int nenv, int device, void* stream, mjh_engine** out) {
  if (!m || nenv <= 0 || !out) { mjh_set_error("mjh_create: bad argument"); return MJH_ERR_ARG; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    mjh_set_error("mjh_create: no HIP device visible (this engine has no CPU fallback)");
    return MJH_ERR_NO_DEVICE;
  }
  if (device < 0 || device >= ndev) { mjh_set_error("mjh_create: bad device index"); return MJH_ERR_ARG; }

  if (m->ngeom > 4095) { mjh_set_error("mjh_create: more than 4095 geoms (contact records pack the geom ids in 12 bits)"); return MJH_ERR_CAPACITY; }
  for (int g = 0; g < m->ngeom; g++) if (m->geom_condim[g] != 1 && m->geom_condim[g] != 3 && m->geom_condim[g] != 4) {
    mjh_set_error("mjh_create: condim must be 1, 3 or 4 (rolling friction, condim 6, is not implemented)"); return MJH_ERR_UNSUPPORTED; }
  HIPCHK(hipSetDevice(device));
  mjh_engine* e = new mjh_engine();
  // from here on every failure path releases the engine and whatever it has allocated so far
#undef HIPCHK
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { mjh_set_error(std::string(#call) + ": " + hipGetErrorString(e_)); mjh_destroy(e); return MJH_ERR_NO_DEVICE; } } while (0)
  if (const char* v = getenv("MJH_LPT")) e->lpt = atoi(v) != 0;
  if (const char* v = getenv("MJH_SPLIT3")) e->split3 = atoi(v) != 0;
  e->model = m; e->nenv = nenv; e->device = device; e->stream = (hipStream_t)stream;

  HostPack hp; derive_fitting(m, hp);
  e->M = hp.M; e->L = hp.L; e->H = hp.H; e->W = hp.W; e->report = hp.report; e->lds_bytes = hp.lds_bytes; e->lds_bytes_pre = hp.lds_bytes_wpre; e->o_controlled = hp.o_controlled; e->o_odom = hp.o_odom;
  DModel& M = e->M; std::vector<int>& I = hp.I; std::vector<float>& F = hp.F;
  e->hI = I;
  if (dev_alloc(e, &e->dI, I.size(), false) || dev_alloc(e, &e->dF, F.size(), false)) { mjh_destroy(e); return MJH_ERR_NO_DEVICE; }
  HIPCHK(hipMemcpyAsync(e->dI, I.data(), I.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->dF, F.data(), F.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  M.I = e->dI; M.F = e->dF;

  if (e->report) {   // contact report: zeros until the first solve
    DReport& R = e->R;
    R.on = 1; R.maxcon = e->M.maxcon; e->split3 = false;      // (the report reads the position stage after the solve: one fused launch)
    if (dev_alloc(e, &R.ncon, (size_t)nenv) || dev_alloc(e, &R.rec, (size_t)nenv * R.maxcon * CREP_STRIDE) || dev_alloc(e, &R.cfrc, (size_t)nenv * 6 * e->M.nbody)) { mjh_destroy(e); return MJH_ERR_NO_DEVICE; }
  }
  {
    DConst hc; hc.M = e->M; hc.L = e->L; hc.H = e->H; hc.W = e->W; hc.R = e->R;
    if (dev_alloc(e, &e->dC, 1, false)) { mjh_destroy(e); return MJH_ERR_NO_DEVICE; }
    HIPCHK(hipMemcpyAsync(e->dC, &hc, sizeof hc, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  if ((long long)(e->M.maxblk - e->M.maxcon) * e->M.rowW + (long long)e->M.maxcon * e->M.rowW * 4 >= 4LL * 65536) {   // hd.x >> 16 holds the offset in float4 units
    mjh_set_error("mjh_create: Jacobian pool too large for the 16-bit block offsets (lower the contact capacity)");
    mjh_destroy(e); return MJH_ERR_CAPACITY;
  }
  if (e->M.big && e->M.rowW > 64) {
    mjh_set_error("mjh_create: nv > 64 needs every constraint to touch at most 64 dofs (this model: " + std::to_string(e->M.rowW) + "); the solver maps one dof of a block per lane");
    mjh_destroy(e); return MJH_ERR_CAPACITY;
  }
  if (e->lds_bytes > 160 * 1024) {
    mjh_set_error("mjh_create: per-env working set exceeds the 160 KiB LDS of one CU (" + std::to_string(e->lds_bytes) + " B)");
    mjh_destroy(e); return MJH_ERR_CAPACITY;
  }
#define MJH_ATTR(NR, DG) do { HIPCHK(hipFuncSetAttribute((const void*)mjh_step_kernel<NR, DG, false>, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes)); \
                              HIPCHK(hipFuncSetAttribute((const void*)mjh_step_kernel<NR, DG, true>, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes)); } while (0)
  if (e->M.dense) {
    // LDS of mjh_dense_build_kernel: 1 / D [nvs] | 1 / AR_qq [cap] | row table [cap] int4 | row starts [maxblk + 1]
    e->dense_lds = ((size_t)e->M.dense_nvs + 5 * (size_t)e->M.dense_cap + (size_t)std::max(e->M.maxblk, 1) + 8) * sizeof(float);
    // ... and of mjh_dense_solve_kernel: start values [cap] | 128 | the factor twice [2 nM] (a 128-dof chain: 67.6 KB, beyond the 64 KB a
    // launch gets without the attribute)
    e->dense_solve_lds = (DN_CAP_MAX + 128 + 2 * (size_t)e->M.nM) * sizeof(float);
    if (e->dense_lds > 160 * 1024 || e->dense_solve_lds > 160 * 1024) { e->M.dense = 0; }
    else {
      HIPCHK(mjh_dense_attributes(e->dense_lds, e->dense_solve_lds));
    }
  }
  MJH_ATTR(1, true); MJH_ATTR(2, true); MJH_ATTR(4, true); MJH_ATTR(8, true); MJH_ATTR(1, false); MJH_ATTR(2, false); MJH_ATTR(4, false); MJH_ATTR(8, false);
#undef MJH_ATTR
  if (e->H.has_hfield) HIPCHK(mjh_step_hf_attributes((size_t)e->lds_bytes));
  if (e->M.window) {
#define MJH_ATTRW(NR, CX, GJ) HIPCHK(hipFuncSetAttribute((const void*)mjh_step_kernel<NR, true, CX, GJ>, hipFuncAttributeMaxDynamicSharedMemorySize, e->lds_bytes))
    MJH_ATTRW(1, false, 1); MJH_ATTRW(1, true, 1); MJH_ATTRW(2, false, 1); MJH_ATTRW(2, true, 1);
    MJH_ATTRW(1, false, 2); MJH_ATTRW(1, true, 2); MJH_ATTRW(2, false, 2); MJH_ATTRW(2, true, 2);
#undef MJH_ATTRW
  }

  // ---- per-env state
  DState& S = e->S;
  const size_t nq_all = (size_t)nenv * M.nqp, nv_all = (size_t)nenv * M.nvp;
  int rc = 0;
  rc |= dev_alloc(e, &S.qpos, nq_all); rc |= dev_alloc(e, &S.initial_qpos, nq_all);
  {   // columns of the per-env record (derive_device_model): qpos | qvel | qacc_warmstart | ddq | dq
    const int nvc = std::max(M.nv, 1);
    S.qvel = S.qpos + M.nq; S.qacc_ws = S.qvel + nvc; S.ddq = S.qacc_ws + nvc; S.dq = S.ddq + nvc;
  }
  S.qacc = S.qacc_ws;   // one array: after every solve qacc_warmstart = qacc (step_kernel.h, store), so the second row would only double the traffic
  rc |= dev_alloc(e, &S.qvel_ref, nv_all); rc |= dev_alloc(e, &S.qfrc_applied, nv_all);
  rc |= dev_alloc(e, &S.qfrc_inverse, nv_all);
  S.gscratch = nullptr; S.gstride = hp.gstride;
  if (M.big) rc |= dev_alloc(e, &S.gscratch, (size_t)nenv * (size_t)hp.gstride, false);   // many-body models: contact / block / Jacobian pools
  S.wbuf = nullptr; S.wstride = 0;
  // (0: off; experiments: another row threshold.  Models whose rows can exceed 256 — S24D — keep every env below the 64-row threshold in the 16-row form:
  //  four envs per wavefront; the two-env wavefronts of the 32-row form cost the SIMD time the one-env wavefronts of the slowest envs need — round 6)
  S.win32 = getenv("MJH_WINDOW32") ? std::max(0, atoi(getenv("MJH_WINDOW32"))) : (M.win_maxw > 16 ? 0 : WN32_MIN_ROWS);
  // 64-row form above ... rows: models whose envs stay within 256 rows (S24: 9 % of the envs beyond 96 rows) give it every env beyond the 16-row
  // form's register-resident windows — 2 x 64 rows with the chains' wait states filled beat 4 x 32 (S24 12.3 -> 13.3 M); models with more rows
  // (S24D: 30 % of the envs between 97 and 128 rows, 60 % beyond) only the envs a cohort's step waits for (176 / 192 / 208 rows: 4.65 / 4.97 / 5.26 M)
  S.win64 = getenv("MJH_WINDOW64") ? std::max(0, atoi(getenv("MJH_WINDOW64"))) : (M.win_maxw > 16 ? WN64_MIN_ROWS : WN32_MIN_ROWS);   // (0: off)
  if (S.win64 > 0 && S.win64 < S.win32) S.win64 = S.win32;
  if (getenv("MJH_WN_NL") && atoi(getenv("MJH_WN_NL")) < 3) S.win64 = 0;      // (experiments that take the LDS tier away: the 64-row section keeps two 16 KB tiles there)
  if (M.window) {   // window sweep: header + vectors + win_maxw windows of rows + tiles of the streamed windows, per env
    S.wj_off = ((WN_ROWS + M.win_maxw * WN_NK * 16 + M.win_maxw * WN_XREC(M.win_nvt) * 16 + (M.win_maxw / 2 + 1) * WN_XPAIR * 16 + 63) / 64) * 64;
    S.wstride = S.wj_off + ((M.win_jsz + 63) / 64) * 64;
    if (((S.wstride / 64) & 1) == 0) S.wstride += 64;      // an odd number of 256-byte lines per env: the same offset of consecutive envs' slices does not fall on the same memory channel
    rc |= dev_alloc(e, &S.wbuf, (size_t)nenv * (size_t)S.wstride, true);
  }
  if (const char* v = getenv("MJH_WINDOW_LEAN")) e->win_lean = atoi(v) != 0;
  if (const char* v = getenv("MJH_WINDOW_STRAIGHT")) e->win_straight = atoi(v) != 0;
  if (M.window && e->lpt && nenv >= 1024) {
    HIPCHK(hipHostMalloc((void**)&e->h_wn, MJH_MAX_COHORTS * sizeof(int), hipHostMallocMapped));
    for (int g = 0; g < MJH_MAX_COHORTS; g++) e->h_wn[g] = 1 << 20;        // (nothing seen yet: keep the LDS tier)
    HIPCHK(hipHostGetDevicePointer((void**)&e->d_wn, e->h_wn, 0));
  }
  if (M.big && M.dense && e->lpt && nenv >= 1024) {
    // one word per cohort in host-mapped memory: "a env of the cohort swept long when its launch order was last rebuilt" (mjh_order_kernel)
    HIPCHK(hipHostMalloc((void**)&e->h_dense, MJH_MAX_COHORTS * 4 * sizeof(int), hipHostMallocMapped));
    for (int g = 0; g < MJH_MAX_COHORTS * 4; g++) e->h_dense[g] = 1;
    for (int g = 0; g < MJH_MAX_COHORTS; g++) e->dense_now[g] = true;
    HIPCHK(hipHostGetDevicePointer((void**)&e->d_dense, e->h_dense, 0));
    for (int g = 0; g < MJH_MAX_COHORTS; g++) for (int k = 0; k < 4; k++) HIPCHK(hipEventCreateWithFlags(&e->ev_dense[g][k], hipEventDisableTiming));
  }
  rc |= dev_alloc(e, &S.time, (size_t)nenv); rc |= dev_alloc(e, &S.odom_vel, (size_t)nenv * 6); rc |= dev_alloc(e, &S.stats, (size_t)nenv * 4);
  rc |= dev_alloc(e, &S.x_bias, nv_all); rc |= dev_alloc(e, &S.x_passive, nv_all); rc |= dev_alloc(e, &S.x_smooth, nv_all);
  rc |= dev_alloc(e, &S.x_constraint, nv_all); rc |= dev_alloc(e, &S.x_energy, (size_t)nenv * 2);
  if (M.nsensor > 0) { rc |= dev_alloc(e, &S.sensordata, (size_t)nenv * 3 * M.nsensor); e->split3 = false; }   // (sensors read the position stage after the solve: one fused launch)
  if (M.nmocap > 0) rc |= dev_alloc(e, &S.mocap, (size_t)nenv * 7 * M.nmocap, false);
  if (rc) { mjh_destroy(e); return MJH_ERR_NO_DEVICE; }
  if (M.nmocap > 0) {   // mocap poses start at the bodies' model poses (d->mocap_pos / mocap_quat after mj_makeData)
    std::vector<float> mp((size_t)nenv * 7 * M.nmocap);
    for (int b = 0; b < m->nbody; b++) if (m->body_mocapid && m->body_mocapid[b] >= 0)
      for (int en = 0; en < nenv; en++) {
        float* p = &mp[((size_t)en * M.nmocap + m->body_mocapid[b]) * 7];
        for (int k = 0; k < 3; k++) p[k] = (float)m->body_pos[3*b+k];
        for (int k = 0; k < 4; k++) p[3+k] = (float)m->body_quat[4*b+k];
      }
    HIPCHK(hipMemcpyAsync(S.mocap, mp.data(), mp.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  // initial state = qpos0 for every env
  {
    std::vector<float> q0(nq_all, 0.0f);
    for (int en = 0; en < nenv; en++) for (int i = 0; i < m->nq; i++) q0[(size_t)en * M.nqp + i] = (float)m->qpos0[i];
    HIPCHK(hipMemcpyAsync(S.qpos, q0.data(), nq_all * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(S.initial_qpos, q0.data(), nq_all * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  // Cohorts: 2 recover ~95% of the slot-limited throughput of the fused step, a third one adds 0 - 9 % there (S24 +1 %, C3 +9 %:
  // not the default, a launch then covers a third of the envs for the same duration);
  // the many-body layout's step is three launches (assemble -> solve -> integrate) and three cohorts keep all three busy (C2 +4 %,
  // C4 +11 %).  Four or more lose (C3 -30 %): streams start to share hardware queues.  Three cohort streams + the caller's stream +
  // the export stream need more than the runtime's default of 4 hardware queues: see mjh_library_init below.
  { int nc = nenv >= 1024 ? (e->M.big && e->split3 && nenv >= 1536 ? 3 : 2) : 1;   // (fused step: two by default, `mjh_set_cohorts(e, 3)` / MJH_COHORTS=3 for the last per cent)
    if (const char* v = getenv("MJH_COHORTS")) nc = atoi(v); if (set_cohorts(e, nc)) { mjh_destroy(e); return MJH_ERR_NO_DEVICE; } }
  *out = e;
  return MJH_OK;
#undef HIPCHK
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { mjh_set_error(std::string(#call) + ": " + hipGetErrorString(e_)); return MJH_ERR_NO_DEVICE; } } while (0)
}

extern "C" void mjh_destroy(mjh_engine* e) {
  if (!e) return;
  (void)join_cohorts(e);
  (void)hipStreamSynchronize(e->stream);
  for (int g = 0; g < MJH_MAX_COHORTS; g++) { if (e->cstream[g]) (void)hipStreamDestroy(e->cstream[g]); if (e->ev_join[g]) (void)hipEventDestroy(e->ev_join[g]); }
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  for (int g = 0; g < MJH_MAX_COHORTS; g++) for (int k = 0; k < 8; k++) if (e->cgraph[g][k].exec) (void)hipGraphExecDestroy(e->cgraph[g][k].exec);
  for (auto& p : e->tev) { (void)hipEventDestroy(p.first); (void)hipEventDestroy(p.second); }
  for (void* p : e->allocs) (void)hipFree(p);
  if (e->scratch) (void)hipFree(e->scratch);
  if (e->ray_io) (void)hipFree(e->ray_io);
  if (e->render_io) (void)hipFree(e->render_io);
  if (e->tex_io) (void)hipFree(e->tex_io);
  if (e->scan_tab) (void)hipFree(e->scan_tab);
  if (e->scan_host) (void)hipHostFree(e->scan_host);
  if (e->scan_up) (void)hipEventDestroy(e->scan_up);
  if (e->hscan_root) (void)hipFree(e->hscan_root);
  if (e->csel_tab) (void)hipFree(e->csel_tab);
  if (e->csel_host) (void)hipHostFree(e->csel_host);
  if (e->csel_up) (void)hipEventDestroy(e->csel_up);
  if (e->csel_io) (void)hipFree(e->csel_io);
  for (mjh_engine::FrameTable* T : {&e->frame_tab, &e->facc_tab}) {
    if (T->tab) (void)hipFree(T->tab);
    if (T->host) (void)hipHostFree(T->host);
    if (T->up) (void)hipEventDestroy(T->up);
  }
  if (e->frame_io) (void)hipFree(e->frame_io);
  if (e->facc_io) (void)hipFree(e->facc_io);
  if (e->rid_host) (void)hipHostFree(e->rid_host);
  if (e->rid_dev) (void)hipFree(e->rid_dev);
  for (int k = 0; k < MJH_IO_SLOTS; k++) if (e->rid_ev[k]) (void)hipEventDestroy(e->rid_ev[k]);
  if (e->h_dense) (void)hipHostFree(e->h_dense);
  if (e->h_wn) (void)hipHostFree(e->h_wn);
  if (e->h_io) (void)hipHostFree(e->h_io);
  for (int k = 0; k < MJH_IO_SLOTS; k++) if (e->io_ev[k]) (void)hipEventDestroy(e->io_ev[k]);
  for (int g = 0; g < MJH_MAX_COHORTS; g++) for (int k = 0; k < 4; k++) if (e->ev_dense[g][k]) (void)hipEventDestroy(e->ev_dense[g][k]);
  delete e;
}

// (every entry point re-selects the engine's device: one process may hold engines on several GPUs, and the caller's
// current device is whatever its framework left it at)
static int flush_step1(mjh_engine* e);
#define ENG_NOJOIN(e) if (!(e)) { mjh_set_error("null engine"); return MJH_ERR_ARG; } \
                      if (hipSetDevice((e)->device) != hipSuccess) { mjh_set_error("hipSetDevice failed"); return MJH_ERR_NO_DEVICE; } \
                      if ((e)->step1_pending) { int rcf_ = flush_step1(e); if (rcf_) return rcf_; } \
                      const bool mjh_ho_ = (e)->handover; (e)->handover = false; (void)mjh_ho_;
// (entry points that cannot change what a pending window hand-over was built from — getters, mjh_set_cmd — put it back)
#define KEEP_HANDOVER(e) (e)->handover = mjh_ho_;
// every entry point except mjh_step first joins the cohort streams back into the caller's stream
#define ENG(e) ENG_NOJOIN(e) { int rcj_ = join_cohorts(e); if (rcj_) return rcj_; }
#define RANGE(e, env0, n) if ((env0) < 0 || (n) < 0 || (env0) + (n) > (e)->nenv) { mjh_set_error("env range out of bounds"); return MJH_ERR_ARG; }

// full-range launch on the caller's stream in longest-job-first order (split API: step1 | inverse | step2 | forward);
// `resort` rebuilds the order from the previous step's solver statistics, otherwise the last order is reused
// With cohorts (mjh_set_cohorts > 1) the range is issued cohort by cohort on the cohort streams, like mjh_step: the reference's loop
// reads and commands ONE environment between the calls (MjHWInterface::read / write, mj_main.cpp:86-106), and only that environment's
// cohort has to wait for the host (mjh_get_joint_state / mjh_set_cmd on a range inside one cohort touch that cohort's stream only).
static int launch_lpt(mjh_engine* e, int ph, int xflags, bool resort, int wmode = 0) {
  const int G = e->ncohort > 1 && e->nenv >= 64 * e->ncohort ? e->ncohort : 1;
  static const bool split_cohorts = !(getenv("MJH_SPLIT_COHORTS") && atoi(getenv("MJH_SPLIT_COHORTS")) == 0);
  if (G > 1 && split_cohorts) {
    if (e->lpt && e->nenv >= 1024 && !e->d_order) { int rc = join_cohorts(e); if (!rc) rc = dev_alloc(e, &e->d_order, (size_t)e->nenv); if (rc) return rc; e->order_valid = false; e->order_G = -1; }
    int rc = fork_cohorts(e);
    if (rc) return rc;
    StateGuard guard(&e->S);
    const bool lpt = e->lpt && e->d_order && e->nenv >= 1024;
    if (lpt) e->S.env_order = e->d_order;
    const int order_every = order_every_of(e);
    const bool sort = lpt && (e->order_G != G || !e->order_valid || (resort && e->order_age % order_every == 0));
    // (the XF_FORCE exports are engine-sized arrays indexed by the row inside the launch's range: shifted to the cohort's first row)
    float* const xb = e->S.x_bias; float* const xp = e->S.x_passive; float* const xs = e->S.x_smooth; float* const xc = e->S.x_constraint; float* const xe = e->S.x_energy;
    for (int g = 0; g < G && !rc; g++) {
      const int g0 = (int)((long long)e->nenv * g / G), g1 = (int)((long long)e->nenv * (g + 1) / G);
      // (window models: the sort also leaves the cohort's largest row count for the window kernel's LDS-tier choice, as in mjh_step —
      //  a host that only ever uses the split API would keep the tier of an engine that has seen nothing yet)
      if (sort) hipLaunchKernelGGL(mjh_order_kernel, dim3(1), dim3(1024), 0, e->cstream[g], (const int*)e->S.stats, e->d_order, g0, g1 - g0, e->d_wn ? e->d_wn + g : (int*)nullptr, e->d_wn ? -1 : 0);
      const size_t o = (size_t)g0 * e->M.nvp;
      e->S.x_bias = xb ? xb + o : nullptr; e->S.x_passive = xp ? xp + o : nullptr; e->S.x_smooth = xs ? xs + o : nullptr;
      e->S.x_constraint = xc ? xc + o : nullptr; e->S.x_energy = xe ? xe + 2 * (size_t)g0 : nullptr;
      e->cur_cohort = g; rc = launch_on(e, e->cstream[g], g0, g1 - g0, 1, ph, xflags, wmode); e->cur_cohort = -1;
    }
    if (sort) { e->order_G = G; e->order_valid = true; }
    return rc;
  }
  { int rc = join_cohorts(e); if (rc) return rc; }
  if (e->lpt && e->nenv >= 1024) {
    if (!e->d_order) { int rc = dev_alloc(e, &e->d_order, (size_t)e->nenv); if (rc) return rc; e->order_valid = false; }
    if (resort || !e->order_valid) {
      hipLaunchKernelGGL(mjh_order_kernel, dim3(1), dim3(1024), 0, e->stream, (const int*)e->S.stats, e->d_order, 0, e->nenv, (int*)nullptr, 0);
      e->order_valid = true; e->order_G = -1;   // (a full-range sort: mjh_step's cohorts must sort their own ranges again)
    }
  }
  StateGuard guard(&e->S);
  if (e->lpt && e->d_order && e->order_valid) e->S.env_order = e->d_order;
  return launch(e, 0, e->nenv, 1, ph, xflags, wmode);
}
static int launch_pd(mjh_engine* e, hipStream_t st, int env0, int n);
// mjh_step1 defers its launch to the next entry point: the reference's loop calls MjHWInterface::read() = mj_inverse right behind
// mj_step1 (mj_main.cpp:83-94), and step1 + inverse as ONE launch share the position and velocity stages (the literal loop's three
// launches per step become two).  Any other entry point first issues the plain step1 launch (ENG / ENG_NOJOIN), so the order of
// effects on the stream is the order of the calls.
// Window chain (small free-body models): the split API's step1 [+ inverse] launch is the chain's ASSEMBLE launch — position and velocity
// stages, controller, [mj_inverse,] and mj_step2's acceleration + constraint rows, handed over in the env's slice; qpos (normalised) and
// qvel (after the controller's velocity override) are stored as mj_step1 leaves them, nothing is integrated — and mjh_step2 is the
// window kernel alone, instead of a second pass over everything the rows need (they only ever exist in LDS).  What the reference's
// loop does between the two (MjHWInterface::read: getters; write: mjh_set_cmd, consumed by the NEXT mj_step1) keeps the hand-over; any
// other call that touches the engine in between drops it, and mjh_step2 runs the whole chain from the state it finds.
static bool split_handover(const mjh_engine* e) {
  static const bool on = !(getenv("MJH_SPLIT_HANDOVER") && atoi(getenv("MJH_SPLIT_HANDOVER")) == 0);
  return on && e->M.window && e->S.wbuf != nullptr;
}
static int flush_step1(mjh_engine* e) {
  e->step1_pending = false;
  if (split_handover(e)) { const int rc = launch_lpt(e, PH_STEP1 | PH_STEP2, XF_FORCE, true, 1); e->handover = rc == MJH_OK; return rc; }
  return launch_lpt(e, PH_STEP1, XF_FORCE, true);
}
extern "C" int mjh_step1(mjh_engine* e) {
  ENG_NOJOIN(e); e->step1_done = true;
  if (e->pd_on) { int rc = join_cohorts(e); if (!rc) rc = launch_pd(e, e->stream, 0, e->nenv); if (rc) return rc; }
  static const bool lazy = !(getenv("MJH_LAZY_STEP1") && atoi(getenv("MJH_LAZY_STEP1")) == 0);
  if (!lazy) return launch_lpt(e, PH_STEP1, XF_FORCE, true);
  e->step1_pending = true;
  return MJH_OK;
}
extern "C" int mjh_inverse(mjh_engine* e) {
  if (e && e->step1_pending) {      // step1 + inverse in one launch
    if (hipSetDevice(e->device) != hipSuccess) { mjh_set_error("hipSetDevice failed"); return MJH_ERR_NO_DEVICE; }
    e->step1_pending = false;
    if (split_handover(e)) { const int rc = launch_lpt(e, PH_STEP1 | PH_INV | PH_STEP2, XF_FORCE, true, 1); e->handover = rc == MJH_OK; return rc; }
    return launch_lpt(e, PH_STEP1 | PH_INV, XF_FORCE, true);
  }
  ENG_NOJOIN(e); return launch_lpt(e, PH_INV, XF_FORCE, false);
}
extern "C" int mjh_step2(mjh_engine* e) {
  ENG_NOJOIN(e);
  if (!e->step1_done) { mjh_set_error("mjh_step2 called before mjh_step1"); return MJH_ERR_STATE; }
  e->step1_done = false;
  e->order_age++;
  if (mjh_ho_) return launch_lpt(e, PH_STEP2, XF_FORCE, false, 2);
  return launch_lpt(e, PH_STEP2, XF_FORCE, false);
}
extern "C" int mjh_forward(mjh_engine* e) {
  ENG(e);
  // mj_forward runs mjcb_control like mj_step1 does, so the in-engine PD law is evaluated in front of it as well
  if (e->pd_on) { int rc = launch_pd(e, e->stream, 0, e->nenv); if (rc) return rc; }
  return launch_lpt(e, PH_STEP1 | PH_NOINT, XF_FORCE, true);
}
extern "C" int mjh_step(mjh_engine* e, int nsteps, int with_inverse) {
  ENG_NOJOIN(e);
  if (e->lpt && !e->d_order && e->nenv >= 1024) {
    int rc = join_cohorts(e);
    if (!rc) rc = dev_alloc(e, &e->d_order, (size_t)e->nenv);
    if (rc) return rc;
  }
  const int G = e->ncohort > 1 && e->nenv >= 64 * e->ncohort ? e->ncohort : 1;
  int rc = G > 1 ? fork_cohorts(e) : join_cohorts(e);
  if (rc) return rc;
  const int ph = PH_STEP1 | PH_STEP2 | (with_inverse ? PH_INV : 0);
  StateGuard guard(&e->S);
  if (e->lpt && e->d_order) e->S.env_order = e->d_order;
  if (e->pd_on && e->pd_target) { e->S.pd_target = e->pd_target; e->S.pd_kp = e->pd_kp; e->S.pd_kd = e->pd_kd; }   // the fused step evaluates the PD law itself
  // In-kernel step loop (step_kernel.h): articulated models in the LDS-resident layout run up to steps_per_launch steps per launch and
  // cohort, the env's state staying in LDS in between (commands are consumed by the first step of the call, the in-engine PD law runs
  // every step); free-body models (contact-patch / window chain) and the many-body chain hand over between launches: one step each
  const int chunk_max = (!e->M.big && !e->M.diagM) ? std::max(1, e->steps_per_launch) : 1;
  for (int s = 0, k = 1; s < nsteps && !rc; s += k, e->order_age += k, e->order_G = G) {
    k = std::min(nsteps - s, chunk_max);
    for (int g = 0; g < G && !rc; g++) {
      const int g0 = (int)((long long)e->nenv * g / G), g1 = (int)((long long)e->nenv * (g + 1) / G);
      hipStream_t st = G > 1 ? e->cstream[g] : e->stream;
      // dispatch the envs with the most solver work first (shorter kernel tail).  An env's cost drifts slowly, so the sort is
      // renewed every MJH_ORDER_EVERY-th step only: its 10 us sit in front of every step launch of the cohort's stream, which
      // is 9 % of a step of the small configs (C3, C5: 0.10 ms kernels)
      const int order_every = order_every_of(e);
      if (e->S.env_order && (e->order_G != G || e->order_age / order_every != (e->order_age - e->last_chunk) / order_every || e->order_age == 0)) {
        const bool dsel = e->M.big && e->split3 && e->M.dense && e->d_dense;
        const unsigned ep = e->dense_epoch[g];
        hipLaunchKernelGGL(mjh_order_kernel, dim3(1), dim3(1024), 0, st, (const int*)e->S.stats, e->d_order, g0, g1 - g0, dsel ? e->d_dense + 4 * g + (ep & 3) : (e->d_wn ? e->d_wn + g : (int*)nullptr), e->d_wn && !dsel ? -1 : e->M.dense_min_iter);
        if (dsel) {
          HIPCHK(hipEventRecord(e->ev_dense[g][ep & 3], st));
          // (this wait bounds how far the host runs ahead of the device for such models: at most two rebuilds of the launch order,
          //  2 x MJH_ORDER_EVERY steps per cohort — INTEGRATION.md §7a)
          if (ep >= 2) { HIPCHK(hipEventSynchronize(e->ev_dense[g][(ep - 2) & 3])); e->dense_now[g] = *(volatile int*)(e->h_dense + 4 * g + ((ep - 2) & 3)) != 0; }
          e->dense_epoch[g] = ep + 1;
        }
      }
      hipEvent_t ta = nullptr, tb = nullptr;
      if (e->timing && (e->timing_count++ % e->timing_stride) == 0) {
        if (e->tev_used == e->tev.size()) { hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b)); e->tev.push_back({a, b}); }
        ta = e->tev[e->tev_used].first; tb = e->tev[e->tev_used].second; e->tev_used++;
        HIPCHK(hipEventRecord(ta, st));
      }
      // the chain of launches of this cohort-step.  dn: dense row-space solver for this cohort's step (the word mjh_order_kernel left two
      // rebuilds of the launch order ago; the assemble launch is TOLD the decision, nothing on the device reads the word); nl: windows of the
      // window kernel's LDS tier (window models: window_tier — an unsynchronised hint read HERE, once per cohort-step)
      const bool chain_big = e->M.big && e->split3;
      const bool chain_win = !chain_big && e->M.window && e->S.wbuf;
      const bool dn = chain_big && e->M.dense && (!e->h_dense || e->dense_now[g]);
      e->cur_cohort = g; const int nl = chain_win ? window_tier(e) : -1; e->cur_cohort = -1;
      auto issue_chain = [&]() -> int {
        int rc = MJH_OK;
        if (e->M.big && e->split3) {
          // many-body layout: assemble -> solve (3 KB of LDS per env instead of ~70 KB: many more resident envs during the
          // sweeps, which are > 90 % of such a step) -> integrate
          // dense row-space solver for this cohort's step?  (the word mjh_order_kernel left two rebuilds of the launch order ago; the
          // assemble launch is TOLD the decision, nothing on the device reads the word)
          rc = launch_on(e, st, g0, g1 - g0, 1, ph | PH_PRE, dn ? XF_DENSE : 0);
          if (!rc && dn) {
            // dense row-space solver (dense_pgs.h): AR = J M^-1 J^T on the matrix cores, then column sweeps, for every env of the
            // launch whose row count fits; the block solver below skips those envs (meta[7])
            HIPCHK(mjh_launch_dense(st, g1 - g0, e->dense_lds, e->dense_solve_lds, e->dC, e->S, g0));
          }
          if (!rc) {
            const size_t lds = (2 * (size_t)(((e->M.nv + 3) / 4) * 4) + 2 * (size_t)std::max(e->M.maxblk, 1) + 4 + 8 + 8 + 8 * (size_t)((e->M.nv + 2) / 3)) * sizeof(float);   // ... + the quad sweep's padded copies (four floats per 3 dofs, twice)   // 2 dof vectors + visiting order + group starts + per-wave partial sums
            const bool xs = e->M.noslip_iterations > 0;      // (the convex narrow phase is not part of the solve launch)
            // wide groups (up to 16 independent blocks) can be shared by several waves per environment (MJH_SOLVE_WAVES = 2, 4: chunk
            // c4 of a group goes to wave c4 % n, a workgroup barrier ends the group).  Measured on C2 (4096 envs, 215 contacts per
            // env): 288 k / 282 k / 259 k env-steps/s with 1 / 2 / 4 waves — the sweep streams 0.4 MB of block operands per env and
            // sweep from L2 / HBM and is bound by that stream, not by the length of the dependent chain; so the default stays 1
            static const int nwave_env = getenv("MJH_SOLVE_WAVES") ? std::max(1, std::min(4, atoi(getenv("MJH_SOLVE_WAVES")))) : 1;
            const dim3 thr(e->M.group_max == 16 && e->M.rowW <= 16 ? 64 * nwave_env : 64);
            if (e->M.diagM) { if (xs) hipLaunchKernelGGL((mjh_solve_kernel<true, true>), dim3(g1 - g0), thr, lds, st, e->dC, e->S, g0);
                              else hipLaunchKernelGGL((mjh_solve_kernel<true, false>), dim3(g1 - g0), thr, lds, st, e->dC, e->S, g0); }
            else { if (xs) hipLaunchKernelGGL((mjh_solve_kernel<false, true>), dim3(g1 - g0), thr, lds, st, e->dC, e->S, g0);
                   else hipLaunchKernelGGL((mjh_solve_kernel<false, false>), dim3(g1 - g0), thr, lds, st, e->dC, e->S, g0); }
            HIPCHK(hipGetLastError());
            rc = launch_on(e, st, g0, g1 - g0, 1, PH_STEP2 | PH_POST, 0);
          }
        } else { e->cur_cohort = g; rc = launch_on(e, st, g0, g1 - g0, k, ph, 0, 0, nl); e->cur_cohort = -1; }
        return rc;
      };
      // One hipGraphLaunch per cohort-step instead of 2 .. 5 kernel launches: the chain is captured once per (cohort, variant) and replayed
      // while nothing its kernels take by value changes (the device-state descriptor, the env range, the phase / tier / dense choice)
      // (not on the NULL stream — it cannot be captured —: small engines without cohort streams on the caller's default stream keep the plain launches)
      if (((chain_big && g_chain_graph >= 1) || (chain_win && g_chain_graph >= 2)) && k == 1 && st != nullptr) {
        const int key = (dn ? 1 : 0) | (with_inverse ? 2 : 0) | ((nl > 0 ? 1 : 0) << 2);
        mjh_engine::ChainGraph& cg = e->cgraph[g][key & 7];
        if (!cg.nocap && (!cg.exec || cg.g0 != g0 || cg.n != g1 - g0 || cg.key != (key | (nl << 8)) || std::memcmp(cg.S, &e->S, sizeof(DState)) != 0)) {
          if (cg.exec) {
            // the retired exec owns the kernel arguments of its launches and mjh_step is asynchronous: its last hipGraphLaunch may still be
            // running on this stream — wait for it before the exec goes (re-capture is rare: a descriptor / range / variant change)
            HIPCHK(hipStreamSynchronize(st));
            (void)hipGraphExecDestroy(cg.exec); cg.exec = nullptr;
          }
          hipGraph_t gr = nullptr;
          if (hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal) == hipSuccess) {
            rc = issue_chain();
            const hipError_t ce = hipStreamEndCapture(st, &gr);        // (always ended, also when a launch inside failed)
            if (!rc && ce != hipSuccess) { mjh_set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(ce)); rc = MJH_ERR_NO_DEVICE; }
            if (!rc && hipGraphInstantiate(&cg.exec, gr, nullptr, nullptr, 0) != hipSuccess) { cg.exec = nullptr; cg.nocap = true; (void)hipGetLastError(); }   // (latched: no capture attempt per step from here on)
            if (gr) (void)hipGraphDestroy(gr);
            if (!rc && cg.exec) { std::memcpy(cg.S, &e->S, sizeof(DState)); cg.g0 = g0; cg.n = g1 - g0; cg.key = key | (nl << 8); }
          } else (void)hipGetLastError();                                // (a stream that cannot be captured: plain launches below)
        }
        if (!rc) { if (cg.exec) { HIPCHK(hipGraphLaunch(cg.exec, st)); e->last_launches = 1; } else { rc = issue_chain(); e->last_launches = chain_big ? (dn ? 5 : 3) : (chain_win ? 2 : 1); } }
      } else { rc = issue_chain(); e->last_launches = chain_big ? (dn ? 5 : 3) : (chain_win ? 2 : 1); }
      if (ta && !rc) HIPCHK(hipEventRecord(tb, st));
    }
    e->last_chunk = k;
  }
  if (e->lpt && e->d_order && nsteps > 0 && !rc) e->order_valid = true;   // the per-cohort sorts tile a full permutation
  return rc;
}
// Per-launch timing of the step kernels with HIP events on the streams they are launched on (bench.py's roofline leg).
// on = 1: every step launch; on = N > 1: every N-th one (a sample: the event pairs themselves cost several microseconds of
// stream time per launch, which shows in launch-bound configs)
extern "C" int mjh_set_launch_timing(mjh_engine* e, int on) { ENG(e); e->timing = on != 0; e->timing_stride = on > 1 ? on : 1; e->timing_count = 0; e->tev_used = 0; return MJH_OK; }
extern "C" int mjh_get_launch_timing(mjh_engine* e, double* mean_ms, int* count) {
  ENG(e);
  HIPCHK(hipStreamSynchronize(e->stream));
  double acc = 0;
  for (size_t i = 0; i < e->tev_used; i++) { float ms = 0; HIPCHK(hipEventElapsedTime(&ms, e->tev[i].first, e->tev[i].second)); acc += ms; }
  if (mean_ms) *mean_ms = e->tev_used ? acc / (double)e->tev_used : 0.0;
  if (count) *count = (int)e->tev_used;
  e->tev_used = 0;
  return MJH_OK;
}
// m->opt.timestep is mutable in the reference: simulate() doubles / halves it when the simulation lags the wall clock
// (mj_main.cpp:150-163).  Takes effect with the next launch.
extern "C" int mjh_set_timestep(mjh_engine* e, double dt) {
  ENG(e);
  if (!(dt > 0)) { mjh_set_error("mjh_set_timestep: dt must be positive"); return MJH_ERR_ARG; }
  e->M.timestep = (float)dt; e->M.timestep_d = dt;
  HIPCHK(hipMemcpyAsync((char*)e->dC + offsetof(DConst, M) + offsetof(DModel, timestep), &e->M.timestep, sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync((char*)e->dC + offsetof(DConst, M) + offsetof(DModel, timestep_d), &e->M.timestep_d, sizeof(double), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}
extern "C" double mjh_get_timestep(const mjh_engine* e) { return e ? e->M.timestep_d : 0.0; }
static int reset_dense_choice(mjh_engine* e);
extern "C" int mjh_set_cohorts(mjh_engine* e, int n) { ENG(e); e->last_launches = 0; int rc = set_cohorts(e, n); return rc ? rc : reset_dense_choice(e); }
extern "C" int mjh_get_cohorts(const mjh_engine* e) { return e ? e->ncohort : 0; }
extern "C" int mjh_launches_per_step(const mjh_engine* e) {
  if (!e) return 0;
  // what the last mjh_step actually queued per cohort-step (1: one captured graph; else the kernel launches of the chain it issued — 3 / 5
  // for the many-body layout's block / dense chain, 2 for the window chain); before the first step: what the next one intends
  if (e->last_launches > 0) return e->last_launches;
  const bool big = e->M.big && e->split3, win = !big && e->M.window && e->S.wbuf;
  const int chain = big ? (e->M.dense ? 5 : 3) : (win ? 2 : 1);
  return ((big && g_chain_graph >= 1) || (win && g_chain_graph >= 2)) ? 1 : chain;
}
extern "C" int mjh_set_steps_per_launch(mjh_engine* e, int n) { ENG(e); e->steps_per_launch = std::max(1, std::min(n, 64)); return MJH_OK; }
extern "C" int mjh_get_steps_per_launch(const mjh_engine* e) { return !e ? 0 : ((!e->M.big && !e->M.diagM) ? e->steps_per_launch : 1); }
extern "C" int mjh_synchronize(mjh_engine* e) { ENG(e); KEEP_HANDOVER(e); HIPCHK(hipStreamSynchronize(e->stream)); return MJH_OK; }

// ---- host <-> device marshalling helpers (double on the host side, padded fp32 rows on the device)
// rows of `width` floats at `stride` floats apart; only the `width` floats are touched (rows may be columns of a wider
// per-env record, see the state layout in mjh_create)
// The stream a transfer of the envs [env0, env0 + n) has to be ordered on: while the cohorts run on their own streams, a range inside
// ONE cohort uses that cohort's stream and leaves the others running; anything else joins them into the caller's stream first.
// rows [env0, env0 + n) of up to three per-env arrays <-> one packed block [n x wa | n x wb | n x wc] in host-mapped memory
__global__ void mjh_gather_rows_kernel(const float* __restrict__ a, int sa, int wa, const float* __restrict__ b, int sb, int wb,
                                       const float* __restrict__ c, int sc, int wc, int env0, int n, float* __restrict__ out) {
  const int na = n * wa, nb = n * wb, nc = n * wc;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < na + nb + nc; i += gridDim.x * blockDim.x) {
    float v;
    if (i < na) v = a[(size_t)(env0 + i / wa) * sa + i % wa];
    else if (i < na + nb) { const int j = i - na; v = b[(size_t)(env0 + j / wb) * sb + j % wb]; }
    else { const int j = i - na - nb; v = c[(size_t)(env0 + j / wc) * sc + j % wc]; }
    out[i] = v;
  }
}
__global__ void mjh_scatter_rows_kernel(const float* __restrict__ in, float* __restrict__ a, int sa, int wa, float* __restrict__ b, int sb, int wb, int env0, int n) {
  const int na = n * wa, nb = n * wb;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < na + nb; i += gridDim.x * blockDim.x) {
    if (i < na) a[(size_t)(env0 + i / wa) * sa + i % wa] = in[i];
    else { const int j = i - na; b[(size_t)(env0 + j / wb) * sb + j % wb] = in[i]; }
  }
}
static int ensure_io(mjh_engine* e) {
  if (e->h_io) return MJH_OK;
  HIPCHK(hipHostMalloc((void**)&e->h_io, (size_t)(MJH_IO_GET_FLOATS + MJH_IO_SLOTS * MJH_IO_PUT_FLOATS) * sizeof(float), hipHostMallocMapped));
  HIPCHK(hipHostGetDevicePointer((void**)&e->d_io, e->h_io, 0));
  for (int k = 0; k < MJH_IO_SLOTS; k++) HIPCHK(hipEventCreateWithFlags(&e->io_ev[k], hipEventDisableTiming));
  return MJH_OK;
}
static int range_stream(mjh_engine* e, int env0, int n, hipStream_t* st) {
  *st = e->stream;
  if (!e->forked) return MJH_OK;
  const int G = e->ncohort;
  if (n > 0 && G > 1 && e->nenv >= 64 * G)
    for (int g = 0; g < G; g++) {
      const int g0 = (int)((long long)e->nenv * g / G), g1 = (int)((long long)e->nenv * (g + 1) / G);
      if (env0 >= g0 && env0 + n <= g1) { *st = e->cstream[g]; return MJH_OK; }
    }
  return join_cohorts(e);
}
static int put_rows(mjh_engine* e, float* dst, int stride, int width, int env0, int n, const double* src, hipStream_t st = nullptr) {
  if (!src || n == 0) return MJH_OK;
  if (!st) st = e->stream;
  std::vector<float> tmp((size_t)n * width);
  for (size_t i = 0; i < tmp.size(); i++) tmp[i] = (float)src[i];
  HIPCHK(hipMemcpy2DAsync(dst + (size_t)env0 * stride, (size_t)stride * sizeof(float), tmp.data(), (size_t)width * sizeof(float),
                          (size_t)width * sizeof(float), (size_t)n, hipMemcpyHostToDevice, st));
  HIPCHK(hipStreamSynchronize(st));
  return MJH_OK;
}
// a column block of wider rows: only `width` floats of every row are written (the rest belongs to other tables)
static int put_cols(mjh_engine* e, float* dst, int stride, int width, int env0, int n, const double* src) { return put_rows(e, dst, stride, width, env0, n, src); }
static int get_rows(mjh_engine* e, const float* src, int stride, int width, int env0, int n, double* dst) {
  if (!dst || n == 0) return MJH_OK;
  std::vector<float> tmp((size_t)n * width);
  HIPCHK(hipMemcpy2DAsync(tmp.data(), (size_t)width * sizeof(float), src + (size_t)env0 * stride, (size_t)stride * sizeof(float),
                          (size_t)width * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < tmp.size(); i++) dst[i] = (double)tmp[i];
  return MJH_OK;
}

extern "C" int mjh_set_cmd(mjh_engine* e, int env0, int n, const double* ddq, const double* dq) {
  ENG_NOJOIN(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  hipStream_t st;
  int rc = range_stream(e, env0, n, &st);
  if (rc) return rc;
  static const bool io_fast = !(getenv("MJH_IO_STAGING") && atoi(getenv("MJH_IO_STAGING")) == 0);
  const int wa = ddq ? e->M.nv : 0, wb = dq ? e->M.nv : 0;
  if (io_fast && n > 0 && wa + wb > 0 && (size_t)n * (wa + wb) <= (size_t)MJH_IO_PUT_FLOATS) {
    // MjHWInterface::write of a few envs: the command goes into the next slot of the host-mapped ring and one small kernel on the
    // range's stream moves it into the per-env records; the call returns without waiting for the device (the slot's event fences
    // its reuse, MJH_IO_SLOTS calls later)
    rc = ensure_io(e);
    if (rc) return rc;
    const unsigned slot = e->io_next++ % MJH_IO_SLOTS;
    if (e->io_used[slot]) HIPCHK(hipEventSynchronize(e->io_ev[slot]));
    float* h = e->h_io + MJH_IO_GET_FLOATS + (size_t)slot * MJH_IO_PUT_FLOATS;
    const size_t na = (size_t)n * wa, nb = (size_t)n * wb;
    for (size_t i = 0; i < na; i++) h[i] = (float)ddq[i];
    for (size_t i = 0; i < nb; i++) h[na + i] = (float)dq[i];
    const int total = (int)(na + nb);
    hipLaunchKernelGGL(mjh_scatter_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const float*)(e->d_io + (h - e->h_io)),
                       wa ? e->S.ddq : e->S.dq, e->M.nvp, wa ? wa : wb, wa ? e->S.dq : nullptr, e->M.nvp, wa ? wb : 0, env0, n);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(e->io_ev[slot], st)); e->io_used[slot] = true;
    return MJH_OK;
  }
  rc = put_rows(e, e->S.ddq, e->M.nvp, e->M.nv, env0, n, ddq, st);
  if (rc) return rc;
  return put_rows(e, e->S.dq, e->M.nvp, e->M.nv, env0, n, dq, st);
}

// ---- device forms (control.hip): dense fp32 rows [n][width] of the caller's device buffers <-> the engine's rows, enqueued on the range's
// stream; no host copy, no conversion, no synchronisation.  The caller orders the buffers' producer / consumer on the engine's stream.
struct RowPart { float* eng; int stride, width; const void* buf; };
static int move_rows(hipStream_t st, int env0, int n, const RowPart* parts, int nparts, bool scatter) {
  ControlRowsArgs A{};
  A.env0 = env0; A.n = n;
  int k = 0;
  for (int i = 0; i < nparts; i++) if (parts[i].buf && parts[i].width > 0) {
    A.eng[k] = parts[i].eng; A.stride[k] = parts[i].stride; A.width[k] = parts[i].width; A.buf[k] = (float*)parts[i].buf; k++;
  }
  if (k == 0 || n <= 0) return MJH_OK;
  HIPCHK(scatter ? mjh_launch_scatter_rows(st, A) : mjh_launch_gather_rows(st, A));
  return MJH_OK;
}
// A move of the rows [env0, env0 + n) that leaves the cohorts forked (commands and the joint state: what a loop issues between two steps).
// Not forked: one launch on the engine's stream.  Forked: every cohort moves its part of the range on its own stream, right behind its last
// step, as mjh_export_state_device does; the caller's buffers are ordered on the engine's stream, so each of those streams is bracketed
// against it — it waits for what the engine's stream holds so far (the buffer's producer), and the engine's stream waits for the move (the
// buffer's consumer, or its release).  Events only, no host wait, and a cohort the range does not touch is left alone.  The rows written are
// those of the joined form.
static int move_rows_forked(mjh_engine* e, int env0, int n, const RowPart* parts, int nparts, bool scatter) {
  const int G = e->ncohort;
  if (!e->forked || G <= 1 || e->nenv < 64 * G) {
    int rc = join_cohorts(e);
    return rc ? rc : move_rows(e->stream, env0, n, parts, nparts, scatter);
  }
  HIPCHK(hipEventRecord(e->ev_fork, e->stream));
  for (int g = 0; g < G; g++) {
    const int g0 = (int)((long long)e->nenv * g / G), g1 = (int)((long long)e->nenv * (g + 1) / G);
    const int lo = std::max(env0, g0), hi = std::min(env0 + n, g1);
    if (lo >= hi) continue;
    RowPart sub[CTL_MAXPART];
    for (int i = 0; i < nparts; i++) {
      sub[i] = parts[i];
      if (sub[i].buf) sub[i].buf = (const float*)sub[i].buf + (size_t)(lo - env0) * (size_t)sub[i].width;
    }
    HIPCHK(hipStreamWaitEvent(e->cstream[g], e->ev_fork, 0));
    int rc = move_rows(e->cstream[g], lo, hi - lo, sub, nparts, scatter);
    if (rc) return rc;
    HIPCHK(hipEventRecord(e->ev_join[g], e->cstream[g]));
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join[g], 0));
  }
  return MJH_OK;
}
extern "C" int mjh_set_cmd_device(mjh_engine* e, int env0, int n, const float* d_ddq, const float* d_dq) {
  ENG_NOJOIN(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  if ((!d_ddq && !d_dq) || n == 0) return MJH_OK;
  const RowPart parts[2] = {{e->S.ddq, e->M.nvp, e->M.nv, d_ddq}, {e->S.dq, e->M.nvp, e->M.nv, d_dq}};
  return move_rows_forked(e, env0, n, parts, 2, true);
}

// ---- in-engine PD effort controller.  The reference runs ros_control effort controllers on the host between read() and
// write() (mj_main.cpp:86-106; gains e.g. PID p 200 d 50, model/ontology/box/box.yaml:5-13) for its ONE environment; with
// thousands of environments that hand-off is a PCIe round trip per step, so the same law can run on the device: in front of
// every step, ddq[d] = kp (target[d] - q[d]) - kd qvel[d] on every hinge / slide dof, consumed by the controller stage of
// step1 exactly like a command written through mjh_set_cmd.
__global__ void mjh_pd_kernel(const DConst* __restrict__ C, const DState S, const float* __restrict__ target, float kp, float kd, int env0, int n) {
  const DModel& M = C->M;
  const int nv = M.nv;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (size_t)n * nv; i += (size_t)gridDim.x * blockDim.x) {
    const int env = env0 + (int)(i / nv), d = (int)(i % nv);
    const int j = M.I[M.o_dof_jntid + d], jt = M.I[M.o_jnt_type + j];
    if (jt != MJH_JNT_HINGE && jt != MJH_JNT_SLIDE) continue;
    const float q = S.qpos[(size_t)env * M.nqp + M.I[M.o_jnt_qposadr + j]], v = S.qvel[(size_t)env * M.nvp + d];
    S.ddq[(size_t)env * M.nvp + d] = kp * (target[(size_t)env * nv + d] - q) - kd * v;
  }
}
static int launch_pd(mjh_engine* e, hipStream_t st, int env0, int n) {
  if (!e->pd_on || !e->pd_target || n <= 0) return MJH_OK;
  const size_t total = (size_t)n * e->M.nv;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
  hipLaunchKernelGGL(mjh_pd_kernel, dim3(blocks), dim3(256), 0, st, e->dC, e->S, (const float*)e->pd_target, e->pd_kp, e->pd_kd, env0, n);
  HIPCHK(hipGetLastError());
  return MJH_OK;
}
extern "C" int mjh_set_pd_controller(mjh_engine* e, double kp, double kd) {
  ENG(e);
  if (kp < 0 || kd < 0) { mjh_set_error("mjh_set_pd_controller: gains must be non-negative"); return MJH_ERR_ARG; }
  if ((kp > 0 || kd > 0) && !e->pd_target) {    // targets start at qpos0 of every dof's joint
    int rc = dev_alloc(e, &e->pd_target, (size_t)e->nenv * std::max(e->M.nv, 1));
    if (rc) return rc;
    const mjh_model* m = e->model;
    std::vector<float> t((size_t)e->nenv * std::max(m->nv, 1), 0.0f);
    for (int en = 0; en < e->nenv; en++) for (int d = 0; d < m->nv; d++) {
      const int j = m->dof_jntid[d];
      if (m->jnt_type[j] == MJH_JNT_HINGE || m->jnt_type[j] == MJH_JNT_SLIDE) t[(size_t)en * m->nv + d] = (float)m->qpos0[m->jnt_qposadr[j]];
    }
    HIPCHK(hipMemcpyAsync(e->pd_target, t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
  }
  e->pd_kp = (float)kp; e->pd_kd = (float)kd; e->pd_on = kp > 0 || kd > 0;
  return MJH_OK;
}
extern "C" int mjh_set_pd_target(mjh_engine* e, int env0, int n, const double* target) {
  ENG(e); RANGE(e, env0, n);
  if (!target) return MJH_ERR_ARG;
  if (!e->pd_target) { mjh_set_error("mjh_set_pd_target: enable the controller first (mjh_set_pd_controller)"); return MJH_ERR_STATE; }
  return put_rows(e, e->pd_target, e->M.nv, e->M.nv, env0, n, target);
}
extern "C" int mjh_set_pd_target_device(mjh_engine* e, int env0, int n, const float* d_target) {
  ENG(e); RANGE(e, env0, n);
  if (!d_target) { mjh_set_error("mjh_set_pd_target_device: null target"); return MJH_ERR_ARG; }
  if (!e->pd_target) { mjh_set_error("mjh_set_pd_target_device: enable the controller first (mjh_set_pd_controller)"); return MJH_ERR_STATE; }
  const RowPart part = {e->pd_target, e->M.nv, e->M.nv, d_target};
  return move_rows(e->stream, env0, n, &part, 1, true);
}

static int patch_int_table(mjh_engine* e, int off, const int* vals, int n) {
  for (int i = 0; i < n; i++) e->hI[off + i] = vals[i];
  HIPCHK(hipMemcpyAsync(e->dI + off, e->hI.data() + off, n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}
extern "C" int mjh_set_controlled_dofs(mjh_engine* e, const int* mask) {
  ENG(e); if (!mask) return MJH_ERR_ARG;
  return patch_int_table(e, e->o_controlled, mask, e->M.nv);
}
extern "C" int mjh_set_odom_dofs(mjh_engine* e, const int lin[3], const int ang[3], const int angq[3]) {
  ENG(e);
  int t[10];
  for (int k = 0; k < 3; k++) { t[k] = lin ? lin[k] : -1; t[3+k] = ang ? ang[k] : -1; t[6+k] = angq ? angq[k] : -1; }
  t[9] = 0; for (int k = 0; k < 6; k++) if (t[k] >= 0) t[9] = 1;
  return patch_int_table(e, e->o_odom, t, 10);
}
extern "C" int mjh_set_odom_vel(mjh_engine* e, int env0, int n, const double* twist) {
  ENG(e); RANGE(e, env0, n);
  return put_rows(e, e->S.odom_vel, 6, 6, env0, n, twist);
}

extern "C" int mjh_get_joint_state(mjh_engine* e, int env0, int n, double* qpos, double* qvel, double* qfrc_inverse) {
  ENG_NOJOIN(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  hipStream_t st;
  int rc = range_stream(e, env0, n, &st);
  if (rc || n == 0) return rc;
  static const bool io_fast = !(getenv("MJH_IO_STAGING") && atoi(getenv("MJH_IO_STAGING")) == 0);
  {
    const int wa = qpos ? e->M.nq : 0, wb = qvel ? e->M.nv : 0, wc = qfrc_inverse ? e->M.nv : 0;
    if (io_fast && wa + wb + wc > 0 && (size_t)n * (wa + wb + wc) <= (size_t)MJH_IO_GET_FLOATS) {
      // MjHWInterface::read of a few envs (once per step of the reference's loop): one small kernel packs the rows into host-mapped
      // memory, ONE synchronisation of the range's stream (33 -> 12 us on an idle engine against three pageable 2D copies)
      rc = ensure_io(e);
      if (rc) return rc;
      const int total = n * (wa + wb + wc);
      hipLaunchKernelGGL(mjh_gather_rows_kernel, dim3((total + 255) / 256), dim3(256), 0, st, (const float*)e->S.qpos, e->M.nqp, wa,
                         (const float*)e->S.qvel, e->M.nvp, wb, (const float*)e->S.qfrc_inverse, e->M.nvp, wc, env0, n, e->d_io);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(st));
      const volatile float* h = e->h_io;
      const size_t na = (size_t)n * wa, nb = (size_t)n * wb, nc = (size_t)n * wc;
      for (size_t i = 0; i < na; i++) qpos[i] = (double)h[i];
      for (size_t i = 0; i < nb; i++) qvel[i] = (double)h[na + i];
      for (size_t i = 0; i < nc; i++) qfrc_inverse[i] = (double)h[na + nb + i];
      return MJH_OK;
    }
  }
  // three strided copies, ONE synchronisation
  const float* src[3] = {e->S.qpos, e->S.qvel, e->S.qfrc_inverse};
  const int stride[3] = {e->M.nqp, e->M.nvp, e->M.nvp}, width[3] = {e->M.nq, e->M.nv, e->M.nv};
  double* dst[3] = {qpos, qvel, qfrc_inverse};
  std::vector<float> tmp[3];
  for (int k = 0; k < 3; k++) {
    if (!dst[k]) continue;
    tmp[k].resize((size_t)n * width[k]);
    HIPCHK(hipMemcpy2DAsync(tmp[k].data(), (size_t)width[k] * sizeof(float), src[k] + (size_t)env0 * stride[k], (size_t)stride[k] * sizeof(float),
                            (size_t)width[k] * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(hipStreamSynchronize(st));
  for (int k = 0; k < 3; k++) if (dst[k]) for (size_t i = 0; i < tmp[k].size(); i++) dst[k][i] = (double)tmp[k][i];
  return MJH_OK;
}
extern "C" int mjh_get_joint_state_device(mjh_engine* e, int env0, int n, float* d_qpos, float* d_qvel, float* d_qfrc_inverse) {
  ENG_NOJOIN(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  if (n == 0 || (!d_qpos && !d_qvel && !d_qfrc_inverse)) return MJH_OK;
  const RowPart parts[3] = {{e->S.qpos, e->M.nqp, e->M.nq, d_qpos}, {e->S.qvel, e->M.nvp, e->M.nv, d_qvel}, {e->S.qfrc_inverse, e->M.nvp, e->M.nv, d_qfrc_inverse}};
  return move_rows_forked(e, env0, n, parts, 3, false);
}

// position-stage recompute for a range of envs with export pointers set
static int fk_export(mjh_engine* e, int env0, int n, double* a, int wa, double* b, int wb, bool geoms) {
  const size_t fa = (size_t)n * wa, fb = (size_t)n * wb;
  int rc = ensure_scratch(e, fa + fb);
  if (rc) return rc;
  {
    StateGuard guard(&e->S);
    if (geoms) { e->S.x_gpos = e->scratch; e->S.x_gmat = e->scratch + fa; } else { e->S.x_xpos = e->scratch; e->S.x_xquat = e->scratch + fa; }
    rc = launch(e, env0, n, 1, PH_FKONLY, geoms ? XF_GEOM : XF_BODY);
  }
  if (rc) return rc;
  if (!rc) rc = get_rows(e, e->scratch, wa, wa, 0, n, a);
  if (!rc) rc = get_rows(e, e->scratch + fa, wb, wb, 0, n, b);
  return rc;
}
extern "C" int mjh_get_body_state(mjh_engine* e, int env0, int n, double* xpos, double* xquat) {
  ENG(e); RANGE(e, env0, n);
  return fk_export(e, env0, n, xpos, 3 * e->M.nbody, xquat, 4 * e->M.nbody, false);
}
extern "C" int mjh_get_geom_state(mjh_engine* e, int env0, int n, double* gpos, double* gmat) {
  ENG(e); RANGE(e, env0, n);
  return fk_export(e, env0, n, gpos, 3 * e->M.ngeom, gmat, 9 * e->M.ngeom, true);
}

extern "C" int mjh_get_state(mjh_engine* e, int env0, int n, double* time, double* qpos, double* qvel, double* ws) {
  ENG(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  int rc = MJH_OK;
  if (time && n) { HIPCHK(hipMemcpyAsync(time, e->S.time + env0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream)); }
  if (!rc) rc = get_rows(e, e->S.qpos, e->M.nqp, e->M.nq, env0, n, qpos);
  if (!rc) rc = get_rows(e, e->S.qvel, e->M.nvp, e->M.nv, env0, n, qvel);
  if (!rc) rc = get_rows(e, e->S.qacc_ws, e->M.nvp, e->M.nv, env0, n, ws);
  return rc;
}
extern "C" int mjh_set_state(mjh_engine* e, int env0, int n, const double* time, const double* qpos, const double* qvel, const double* ws) {
  ENG(e); RANGE(e, env0, n);
  int rc = MJH_OK;
  if (time && n) { HIPCHK(hipMemcpyAsync(e->S.time + env0, time, (size_t)n * sizeof(double), hipMemcpyHostToDevice, e->stream)); HIPCHK(hipStreamSynchronize(e->stream)); }
  if (!rc) rc = put_rows(e, e->S.qpos, e->M.nqp, e->M.nq, env0, n, qpos);
  if (!rc) rc = put_rows(e, e->S.qvel, e->M.nvp, e->M.nv, env0, n, qvel);
  if (!rc) rc = put_rows(e, e->S.qacc_ws, e->M.nvp, e->M.nv, env0, n, ws);
  return rc;
}

// add_old_state() (mj_sim.cpp:465-558) for all environments at once: host-side gather / scatter between two engines
extern "C" int mjh_transplant_state(mjh_engine* from, mjh_engine* to, int qpos_mode) {
  if (!from || !to || from == to) { mjh_set_error("mjh_transplant_state: bad engines"); return MJH_ERR_ARG; }
  const mjh_model *ma = from->model, *mb = to->model;
  const int n = std::min(from->nenv, to->nenv);
  static const int QN[4] = {7, 4, 1, 1};
  const size_t nqa = ma->nq, nva = ma->nv, nqb = mb->nq, nvb = mb->nv;
  std::vector<double> ta(n), qa(n * nqa), va(n * nva), wa(n * nva), fa(n * nva), aa(n * nva);
  std::vector<double> tb(n), qb(n * nqb), vb(n * nvb), wb(n * nvb), fb(n * nvb), ab(n * nvb);
  int rc = mjh_get_state(from, 0, n, ta.data(), qa.data(), va.data(), wa.data());
  if (!rc) rc = mjh_get_field(from, "qfrc_applied", 0, n, fa.data());
  if (!rc) rc = mjh_get_field(from, "qacc", 0, n, aa.data());
  if (!rc) rc = mjh_get_state(to, 0, n, tb.data(), qb.data(), vb.data(), wb.data());
  if (!rc) rc = mjh_get_field(to, "qfrc_applied", 0, n, fb.data());
  if (!rc) rc = mjh_get_field(to, "qacc", 0, n, ab.data());
  if (rc) return rc;
  // d_new->xfrc_applied[body] = d->xfrc_applied[body] (mj_sim.cpp:496-500), if the old engine carries any
  std::vector<double> xa, xb;
  const bool has_x = from->S.xfrc_applied != nullptr;
  if (has_x) {
    xa.resize((size_t)n * 6 * ma->nbody); xb.assign((size_t)n * 6 * mb->nbody, 0.0);
    rc = mjh_get_xfrc_applied(from, 0, n, xa.data());
    if (!rc) rc = mjh_get_xfrc_applied(to, 0, n, xb.data());
    if (rc) return rc;
  }
  int matched = 0;
  for (int ba = 1; ba < ma->nbody; ba++) {
    const char* name = ma->body_names ? ma->body_names[ba] : nullptr;
    if (!name || !*name) continue;
    const int bb = mjh_name2id(mb, 0, name);
    if (bb <= 0) continue;
    matched++;
    if (has_x) for (int i = 0; i < n; i++) for (int k = 0; k < 6; k++) xb[((size_t)i * mb->nbody + bb) * 6 + k] = xa[((size_t)i * ma->nbody + ba) * 6 + k];
    const int ja = ma->body_jntnum[ba], jb = mb->body_jntnum[bb];
    if (ja == jb && ja > 0) {
      const int pa = ma->jnt_qposadr[ma->body_jntadr[ba]], pb = mb->jnt_qposadr[mb->body_jntadr[bb]];
      int cnt = ja;                                   // literal: one scalar per joint (mj_sim.cpp:510-513)
      if (qpos_mode) { cnt = 0; for (int j = 0; j < ja; j++) cnt += QN[ma->jnt_type[ma->body_jntadr[ba] + j]]; }
      bool same = true;
      for (int j = 0; j < ja; j++) same &= ma->jnt_type[ma->body_jntadr[ba] + j] == mb->jnt_type[mb->body_jntadr[bb] + j];
      if (same || !qpos_mode)
        for (int i = 0; i < n; i++) for (int k = 0; k < cnt; k++) qb[i * nqb + pb + k] = qa[i * nqa + pa + k];
    }
    const int da = ma->body_dofnum[ba], db = mb->body_dofnum[bb];
    if (da == db && da > 0) {
      const int oa = ma->body_dofadr[ba], ob = mb->body_dofadr[bb];
      for (int i = 0; i < n; i++) for (int k = 0; k < da; k++) {
        vb[i * nvb + ob + k] = va[i * nva + oa + k]; wb[i * nvb + ob + k] = wa[i * nva + oa + k];
        fb[i * nvb + ob + k] = fa[i * nva + oa + k]; ab[i * nvb + ob + k] = aa[i * nva + oa + k];
      }
    }
  }
  for (int i = 0; i < n; i++) tb[i] = ta[i];          // d_new->time = d->time
  rc = put_rows(to, to->S.qacc, to->M.nvp, to->M.nv, 0, n, ab.data());      // (qacc shares its array with qacc_warmstart, which is written next)
  if (!rc) rc = mjh_set_state(to, 0, n, tb.data(), qb.data(), vb.data(), wb.data());
  if (!rc) rc = put_rows(to, to->S.qfrc_applied, to->M.nvp, to->M.nv, 0, n, fb.data());
  if (!rc && has_x) rc = mjh_set_xfrc_applied(to, 0, n, xb.data());
  return rc ? rc : matched;
}

extern "C" int mjh_get_field(mjh_engine* e, const char* name, int env0, int n, double* out) {
  ENG(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  if (!name) return MJH_ERR_ARG;
  const std::string s(name);
  const int nvp = e->M.nvp, nv = e->M.nv;
  if (s == "qacc") return get_rows(e, e->S.qacc, nvp, nv, env0, n, out);
  if (s == "qfrc_bias") return get_rows(e, e->S.x_bias, nvp, nv, env0, n, out);
  if (s == "qfrc_passive") return get_rows(e, e->S.x_passive, nvp, nv, env0, n, out);
  if (s == "qacc_smooth") return get_rows(e, e->S.x_smooth, nvp, nv, env0, n, out);
  if (s == "qfrc_constraint") return get_rows(e, e->S.x_constraint, nvp, nv, env0, n, out);
  if (s == "qfrc_applied") return get_rows(e, e->S.qfrc_applied, nvp, nv, env0, n, out);
  if (s == "qfrc_inverse") return get_rows(e, e->S.qfrc_inverse, nvp, nv, env0, n, out);
  if (s == "qacc_warmstart") return get_rows(e, e->S.qacc_ws, nvp, nv, env0, n, out);
  if (s == "energy") return get_rows(e, e->S.x_energy, 2, 2, env0, n, out);
  mjh_set_error("mjh_get_field: unknown field " + s);
  return MJH_ERR_ARG;
}

extern "C" int mjh_get_stats(mjh_engine* e, int env0, int n, int* out) {
  ENG(e); KEEP_HANDOVER(e); RANGE(e, env0, n);
  HIPCHK(hipMemcpyAsync(out, e->S.stats + (size_t)env0 * 4, (size_t)n * 4 * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; i++) out[4*i + 3] &= 0xff;   // (bits 8.. : the kernel's cost hint for the launch order, not a flag)
  return MJH_OK;
}

extern "C" int mjh_get_contacts(mjh_engine* e, int env, double* dist, double* pos, double* frame, int* geom) {
  ENG(e); RANGE(e, env, 1);
  const int mc = e->M.maxcon;
  int rc = ensure_scratch(e, (size_t)mc * CON_STRIDE + 4);
  if (rc) return rc;
  {
    // read-only snapshot: position stage up to the collision stage, the records and their count go to the scratch buffer
    // and the launch ends there (XF_NOSTORE): state, statistics, time and warm start of the env are not touched
    StateGuard guard(&e->S);
    e->S.x_contacts = e->scratch;
    rc = launch(e, env, 1, 1, 0, XF_CON | XF_NOSTORE, (e->M.window && e->S.wbuf) ? 3 : 0);
  }
  if (rc) return rc;
  std::vector<float> tmp((size_t)mc * CON_STRIDE + 4);
  HIPCHK(hipMemcpyAsync(tmp.data(), e->scratch, tmp.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  int ncon; std::memcpy(&ncon, tmp.data() + (size_t)mc * CON_STRIDE, 4);
  for (int c = 0; c < ncon; c++) {
    const float* r = tmp.data() + (size_t)c * CON_STRIDE;
    if (dist) dist[c] = r[0];
    if (pos) for (int k = 0; k < 3; k++) pos[3*c+k] = r[1+k];
    if (frame) for (int k = 0; k < 9; k++) frame[9*c+k] = r[4+k];
    if (geom) { int g; std::memcpy(&g, r + CON_GEOMS, 4); geom[2*c] = g & 0xfff; geom[2*c+1] = (g >> 12) & 0xfff; }
  }
  return ncon;
}

extern "C" int mjh_mulM(mjh_engine* e, int env0, int n, const double* vec, double* res) {
  ENG(e); RANGE(e, env0, n);
  if (!vec || !res) return MJH_ERR_ARG;
  const int nvp = e->M.nvp;
  int rc = ensure_scratch(e, (size_t)2 * n * nvp);
  if (rc) return rc;
  rc = put_rows(e, e->scratch, nvp, e->M.nv, 0, n, vec);
  if (rc) return rc;
  {
    StateGuard guard(&e->S);
    e->S.x_vec = e->scratch; e->S.x_res = e->scratch + (size_t)n * nvp;
    rc = launch(e, env0, n, 1, PH_MULM, 0);
  }
  if (rc) return rc;
  return get_rows(e, e->scratch + (size_t)n * nvp, nvp, e->M.nv, 0, n, res);
}

extern "C" int mjh_set_env_param(mjh_engine* e, int which, int env0, int n, const double* values) {
  ENG(e); RANGE(e, env0, n);
  if (which < 0 || which >= MJH_EP_COUNT || !values) return MJH_ERR_ARG;
  const mjh_model* m = e->model;
  const int widths[MJH_EP_COUNT] = {3 * m->ngeom, m->ngeom, m->nbody, 3 * m->nbody, 2 * m->nbody, m->nv};
  const double* defaults[MJH_EP_COUNT] = {m->geom_size, m->geom_rbound, m->body_mass, m->body_inertia, m->body_invweight0, m->dof_invweight0};
  const int w = widths[which];
  if (!e->p_tables[0]) {
    // first use: ONE array with a row per env holding all six tables back to back (rows padded to 64 B), every table
    // initialised with the shared model's values; the six device pointers address their column of it
    int off[MJH_EP_COUNT], total = 0;
    for (int k = 0; k < MJH_EP_COUNT; k++) { off[k] = total; total += widths[k]; }
    const int P = ((total + 15) / 16) * 16;
    float* p = nullptr;
    int rc = dev_alloc(e, &p, (size_t)e->nenv * P, false);
    if (rc) return rc;
    std::vector<float> init((size_t)e->nenv * P, 0.0f);
    for (int en = 0; en < e->nenv; en++) for (int k = 0; k < MJH_EP_COUNT; k++) for (int i = 0; i < widths[k]; i++) init[(size_t)en * P + off[k] + i] = (float)defaults[k][i];
    HIPCHK(hipMemcpyAsync(p, init.data(), init.size() * sizeof(float), hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipStreamSynchronize(e->stream));
    const float** slots[MJH_EP_COUNT] = {&e->S.p_geom_size, &e->S.p_geom_rbound, &e->S.p_body_mass, &e->S.p_body_inertia, &e->S.p_body_invweight0, &e->S.p_dof_invweight0};
    for (int k = 0; k < MJH_EP_COUNT; k++) { e->p_tables[k] = p + off[k]; *slots[k] = p + off[k]; }
    e->S.p_stride = P;
  }
  return put_cols(e, e->p_tables[which], e->S.p_stride, w, env0, n, values);
}

// d->xfrc_applied (mj_sim.cpp:499): force + torque per body at its centre of mass, world frame
// first use: the zeroed per-env array (from then on the engine takes the EXTRA instances of the step kernel); waits for the device once
static int ensure_xfrc(mjh_engine* e) {
  if (e->S.xfrc_applied) return MJH_OK;
  const int w = 6 * e->M.nbody;
  const int stride = ((w + 3) / 4) * 4;
  int rc = dev_alloc(e, &e->S.xfrc_applied, (size_t)e->nenv * stride);
  if (rc) return rc;
  HIPCHK(hipStreamSynchronize(e->stream));
  e->S.xfrc_stride = stride;
  return MJH_OK;
}
extern "C" int mjh_set_xfrc_applied(mjh_engine* e, int env0, int n, const double* xfrc) {
  ENG(e); RANGE(e, env0, n);
  if (!xfrc) return MJH_ERR_ARG;
  int rc = ensure_xfrc(e);
  if (rc) return rc;
  return put_rows(e, e->S.xfrc_applied, e->S.xfrc_stride, 6 * e->M.nbody, env0, n, xfrc);
}
extern "C" int mjh_set_xfrc_applied_device(mjh_engine* e, int env0, int n, const float* d_xfrc) {
  ENG(e); RANGE(e, env0, n);
  if (!d_xfrc) { mjh_set_error("mjh_set_xfrc_applied_device: null xfrc"); return MJH_ERR_ARG; }
  int rc = ensure_xfrc(e);
  if (rc) return rc;
  const RowPart part = {e->S.xfrc_applied, e->S.xfrc_stride, 6 * e->M.nbody, d_xfrc};
  return move_rows(e->stream, env0, n, &part, 1, true);
}
extern "C" int mjh_get_xfrc_applied(mjh_engine* e, int env0, int n, double* xfrc) {
  ENG(e); RANGE(e, env0, n);
  if (!xfrc) return MJH_ERR_ARG;
  const int w = 6 * e->M.nbody;
  if (!e->S.xfrc_applied) { std::memset(xfrc, 0, (size_t)n * w * sizeof(double)); return MJH_OK; }
  return get_rows(e, e->S.xfrc_applied, e->S.xfrc_stride, w, env0, n, xfrc);
}
// d->sensordata as mj_step2's mj_sensorAcc left it (the reference's publisher reads it unlocked at its own rate, mj_ros.cpp:1933-1966)
extern "C" int mjh_get_sensordata(mjh_engine* e, int env0, int n, double* out) {
  ENG(e); RANGE(e, env0, n);
  if (!out) return MJH_ERR_ARG;
  if (e->M.nsensor == 0) return MJH_OK;
  return get_rows(e, e->S.sensordata, 3 * e->M.nsensor, 3 * e->M.nsensor, env0, n, out);
}
// d->mocap_pos / d->mocap_quat of one mocap body for a range of environments
extern "C" int mjh_set_mocap_pose(mjh_engine* e, int env0, int n, int mocapid, const double* pos, const double* quat) {
  ENG(e); RANGE(e, env0, n);
  if (mocapid < 0 || mocapid >= e->M.nmocap) { mjh_set_error("mjh_set_mocap_pose: no such mocap body"); return MJH_ERR_ARG; }
  const int stride = 7 * e->M.nmocap;
  if (pos) { int rc = put_rows(e, e->S.mocap + 7 * mocapid, stride, 3, env0, n, pos); if (rc) return rc; }
  if (quat) {
    std::vector<double> q((size_t)n * 4);
    for (int i = 0; i < n; i++) {       // stored normalised (mj_kinematics normalises mocap_quat on use)
      const double* s = quat + 4 * (size_t)i; double nn = std::sqrt(s[0]*s[0] + s[1]*s[1] + s[2]*s[2] + s[3]*s[3]);
      if (!(nn > 1e-12)) { mjh_set_error("mjh_set_mocap_pose: zero quaternion"); return MJH_ERR_ARG; }
      for (int k = 0; k < 4; k++) q[4 * (size_t)i + k] = s[k] / nn;
    }
    return put_rows(e, e->S.mocap + 7 * mocapid + 3, stride, 4, env0, n, q.data());
  }
  return MJH_OK;
}

extern "C" int mjh_set_initial_qpos(mjh_engine* e, int env0, int n, const double* qpos) {
  ENG(e); RANGE(e, env0, n);
  return put_rows(e, e->S.initial_qpos, e->M.nqp, e->M.nq, env0, n, qpos);
}

// The per-cohort dense / block solver choice (the words mjh_order_kernel leaves in host-mapped memory, adopted two sorts later) is part of
// what a run from reset reproduces: a full reset and a new cohort split start it over (dense for everyone, epoch 0, launch order renewed).
// Drains the stream: the order kernels in flight still write the words.
static int reset_dense_choice(mjh_engine* e) {
  if (!e->h_dense) return MJH_OK;
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int g = 0; g < MJH_MAX_COHORTS * 4; g++) e->h_dense[g] = 1;
  for (int g = 0; g < MJH_MAX_COHORTS; g++) { e->dense_now[g] = true; e->dense_epoch[g] = 0; }
  e->order_age = 0; e->order_G = -1;
  return MJH_OK;
}
// ids (already checked against nenv) -> next pinned slot -> the device buffer -> one launch of the reset kernel, all on the caller's stream.
// A slot is rewritten MJH_IO_SLOTS calls later, after its event (the end of its upload); the device buffer is rewritten in stream order.
static int reset_id_list(mjh_engine* e, const int* ids, int n) {
  if ((size_t)n > e->rid_cap) {
    size_t cap = 1024;
    while (cap < (size_t)n) cap *= 2;
    if (e->rid_host) {      // (uploads and launches in flight still read the old buffers)
      HIPCHK(hipStreamSynchronize(e->stream));
      HIPCHK(hipHostFree(e->rid_host)); e->rid_host = nullptr;
      HIPCHK(hipFree(e->rid_dev)); e->rid_dev = nullptr;
      e->rid_cap = 0;
      for (int k = 0; k < MJH_IO_SLOTS; k++) e->rid_used[k] = false;
    }
    HIPCHK(hipHostMalloc((void**)&e->rid_host, (size_t)MJH_IO_SLOTS * cap * sizeof(int), hipHostMallocDefault));
    HIPCHK(hipMalloc((void**)&e->rid_dev, cap * sizeof(int)));
    for (int k = 0; k < MJH_IO_SLOTS; k++) if (!e->rid_ev[k]) HIPCHK(hipEventCreateWithFlags(&e->rid_ev[k], hipEventDisableTiming));
    e->rid_cap = cap;
  }
  const unsigned slot = e->rid_next++ % MJH_IO_SLOTS;
  if (e->rid_used[slot]) HIPCHK(hipEventSynchronize(e->rid_ev[slot]));
  int* const h = e->rid_host + (size_t)slot * e->rid_cap;
  std::memcpy(h, ids, (size_t)n * sizeof(int));
  HIPCHK(hipMemcpyAsync(e->rid_dev, h, (size_t)n * sizeof(int), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipEventRecord(e->rid_ev[slot], e->stream)); e->rid_used[slot] = true;
  ControlResetArgs A{};
  A.C = e->dC; A.S = e->S; A.ids = e->rid_dev; A.env0 = 0; A.n = n;
  HIPCHK(mjh_launch_reset_rows(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_reset(mjh_engine* e, const int* env_ids, int n) {
  ENG(e);
  if (!env_ids) {
    if (e->h_wn) for (int g = 0; g < MJH_MAX_COHORTS; g++) e->h_wn[g] = 1 << 20;     // (row counts of the old state: keep the window kernel's LDS tier until the next look)
    int rc = reset_dense_choice(e); return rc ? rc : launch(e, 0, e->nenv, 1, PH_RESET, 0);
  }
  if (n >= 2) {
    // a list: checked as a whole, then ONE upload and ONE launch of the reset kernel (control.hip) instead of a launch of the step kernel per id
    for (int i = 0; i < n; i++) if (env_ids[i] < 0 || env_ids[i] >= e->nenv) { mjh_set_error("mjh_reset: env id out of range"); return MJH_ERR_ARG; }
    return reset_id_list(e, env_ids, n);
  }
  for (int i = 0; i < n; i++) {
    if (env_ids[i] < 0 || env_ids[i] >= e->nenv) { mjh_set_error("mjh_reset: env id out of range"); return MJH_ERR_ARG; }
    int rc = launch(e, env_ids[i], 1, 1, PH_RESET, 0);
    if (rc) return rc;
  }
  return MJH_OK;
}
// Masked reset of a range from device buffers: every env of [env0, env0 + n) with d_mask[i] != 0 (all of them without a mask) gets what
// mjh_reset does to one env, its qpos / qvel row from d_qpos / d_qvel where given; the others are neither read nor written.  Like mjh_reset
// with an id list it leaves launch order, dense choice and h_wn alone; it drops a pending hand-over (the state it was built from changes).
extern "C" int mjh_reset_device(mjh_engine* e, int env0, int n, const unsigned char* d_mask, const float* d_qpos, const float* d_qvel) {
  ENG(e); RANGE(e, env0, n);
  if (n == 0) return MJH_OK;
  ControlResetArgs A{};
  A.C = e->dC; A.S = e->S; A.mask = d_mask; A.ids = nullptr; A.qpos = d_qpos; A.qvel = d_qvel; A.env0 = env0; A.n = n;
  HIPCHK(mjh_launch_reset_rows(e->stream, A));
  return MJH_OK;
}

// spawn/destroy as batched slot re-layout (reference: spawn_objects / destroy_objects,
// mj_ros.cpp:906-1507 -> full XML round trip + recompile): a pre-allocated free body is toggled per env.
extern "C" int mjh_set_slot_active(mjh_engine* e, int env0, int n, int body, int active) {
  ENG(e); RANGE(e, env0, n);
  const int sbase = e->M.nbody > 32 ? e->M.nbody - 32 : 0;     // the last 32 bodies of a big model are the toggleable slots
  if (body <= 0 || body >= e->M.nbody || body < sbase) {
    mjh_set_error("mjh_set_slot_active: body must be one of the last 32 bodies, [" + std::to_string(std::max(1, sbase)) + ", " + std::to_string(e->M.nbody) + ")");
    return MJH_ERR_ARG;
  }
  const int bit = body - sbase;
  if (!e->S.slot_mask) { int rc = dev_alloc(e, &e->S.slot_mask, (size_t)e->nenv); if (rc) return rc; }
  std::vector<unsigned> h(n);
  HIPCHK(hipMemcpyAsync(h.data(), e->S.slot_mask + env0, n * sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; i++) h[i] = active ? (h[i] & ~(1u << bit)) : (h[i] | (1u << bit));
  HIPCHK(hipMemcpyAsync(e->S.slot_mask + env0, h.data(), n * sizeof(unsigned), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}
// Batched spawn / destroy: the reference's services take a LIST of objects per call (spawn_objects / destroy_objects,
// mj_ros.cpp:859-904,1430-1507); with many environments one call carries (env, body) pairs and the whole list goes to the device
// in one upload + one small kernel instead of three copies and syncs per object.
__global__ void mjh_slot_kernel(const DConst* __restrict__ C, const DState S, const int* __restrict__ env, const int* __restrict__ body,
                                const float* __restrict__ pose /* [n][13] pos3 quat4 vel6, or null: destroy */, int n, int sbase,
                                const int* __restrict__ qadr, const int* __restrict__ dadr) {
  const DModel& M = C->M;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int e = env[i], b = body[i];
  const unsigned bit = 1u << (b - sbase);
  if (pose) {
    atomicAnd(&S.slot_mask[e], ~bit);
    const float* p = pose + 13 * (size_t)i;
    float* q = S.qpos + (size_t)e * M.nqp + qadr[i]; float* v = S.qvel + (size_t)e * M.nvp + dadr[i];
    for (int k = 0; k < 7; k++) q[k] = p[k];
    for (int k = 0; k < 6; k++) v[k] = p[7 + k];
  } else atomicOr(&S.slot_mask[e], bit);
}
static int slot_batch(mjh_engine* e, int n, const int* env, const int* body, const double* pos, const double* quat, const double* vel, bool spawn) {
  if (n <= 0) return MJH_OK;
  if (!env || !body || (spawn && !pos)) { mjh_set_error("mjh_spawn/destroy_objects: null argument"); return MJH_ERR_ARG; }
  const mjh_model* m = e->model;
  const int sbase = e->M.nbody > 32 ? e->M.nbody - 32 : 0;
  std::vector<int> ib(4 * (size_t)n);     // env | body | qpos address | dof address
  std::vector<float> fp(spawn ? 13 * (size_t)n : 0);
  for (int i = 0; i < n; i++) {
    const int b = body[i];
    if (env[i] < 0 || env[i] >= e->nenv || b <= 0 || b >= m->nbody || b < sbase) { mjh_set_error("mjh_spawn/destroy_objects: env or body out of range (slots are the last 32 bodies)"); return MJH_ERR_ARG; }
    ib[i] = env[i]; ib[n + i] = b;
    if (spawn) {
      if (m->body_jntnum[b] != 1 || m->jnt_type[m->body_jntadr[b]] != MJH_JNT_FREE) { mjh_set_error("mjh_spawn_objects: not a free body"); return MJH_ERR_ARG; }
      ib[2 * (size_t)n + i] = m->jnt_qposadr[m->body_jntadr[b]]; ib[3 * (size_t)n + i] = m->body_dofadr[b];
      float* p = &fp[13 * (size_t)i];
      for (int k = 0; k < 3; k++) p[k] = (float)pos[3 * (size_t)i + k];
      for (int k = 0; k < 4; k++) p[3 + k] = (float)(quat ? quat[4 * (size_t)i + k] : (k == 0));
      for (int k = 0; k < 6; k++) p[7 + k] = (float)(vel ? vel[6 * (size_t)i + k] : 0.0);
    }
  }
  if (!e->S.slot_mask) { int rc = dev_alloc(e, &e->S.slot_mask, (size_t)e->nenv); if (rc) return rc; }
  DevBuf di, df;
  HIPCHK(hipMalloc(&di.p, ib.size() * sizeof(int)));
  HIPCHK(hipMemcpyAsync(di.p, ib.data(), ib.size() * sizeof(int), hipMemcpyHostToDevice, e->stream));
  if (spawn) { HIPCHK(hipMalloc(&df.p, fp.size() * sizeof(float))); HIPCHK(hipMemcpyAsync(df.p, fp.data(), fp.size() * sizeof(float), hipMemcpyHostToDevice, e->stream)); }
  const int* d = (const int*)di.p;
  hipLaunchKernelGGL(mjh_slot_kernel, dim3((n + 127) / 128), dim3(128), 0, e->stream, e->dC, e->S, d, d + n, (const float*)df.p, n, sbase, d + 2 * (size_t)n, d + 3 * (size_t)n);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(e->stream));      // (the temporaries are freed on return)
  return MJH_OK;
}
extern "C" int mjh_spawn_objects(mjh_engine* e, int n, const int* env, const int* body, const double* pos, const double* quat, const double* vel) {
  ENG(e); return slot_batch(e, n, env, body, pos, quat, vel, true);
}
extern "C" int mjh_destroy_objects(mjh_engine* e, int n, const int* env, const int* body) {
  ENG(e); return slot_batch(e, n, env, body, nullptr, nullptr, nullptr, false);
}
// pose + twist of one free body of one env (initial state of a spawned object, mj_ros.cpp:1406-1412)
extern "C" int mjh_set_body_pose(mjh_engine* e, int env, int body, const double pos[3], const double quat[4], const double vel[6]) {
  ENG(e); RANGE(e, env, 1);
  const mjh_model* m = e->model;
  if (body <= 0 || body >= m->nbody || m->body_jntnum[body] != 1 || m->jnt_type[m->body_jntadr[body]] != MJH_JNT_FREE) {
    mjh_set_error("mjh_set_body_pose: not a free body"); return MJH_ERR_ARG; }
  const int qa = m->jnt_qposadr[m->body_jntadr[body]], da = m->body_dofadr[body];
  float q[7], v[6];
  for (int k = 0; k < 3; k++) q[k] = (float)pos[k];
  for (int k = 0; k < 4; k++) q[3+k] = (float)(quat ? quat[k] : (k == 0));
  for (int k = 0; k < 6; k++) v[k] = (float)(vel ? vel[k] : 0.0);
  HIPCHK(hipMemcpyAsync(e->S.qpos + (size_t)env * e->M.nqp + qa, q, sizeof q, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipMemcpyAsync(e->S.qvel + (size_t)env * e->M.nvp + da, v, sizeof v, hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}

// ---- pinned host mirror of a range of environments: what the reference's publisher threads read from
// mjData (mj_ros.cpp:1968-2194: qpos / qvel / qfrc_inverse for joint states, xpos / xquat for tf and object states,
// geom_xpos / geom_xmat for markers), refreshed asynchronously at each topic's rate instead of per step.
struct mjh_mirror {
  mjh_engine* e = nullptr; int env0 = 0, n = 0;
  float* host = nullptr; float* dev = nullptr;          // pinned block / device staging of the FK exports
  size_t off[8] = {0}; int width[8] = {0}; size_t total = 0, fk_floats = 0;
  hipEvent_t ev = nullptr;
};
extern "C" int mjh_mirror_create(mjh_engine* e, int env0, int n, mjh_mirror** out) {
  ENG(e); RANGE(e, env0, n);
  if (!out || n <= 0) { mjh_set_error("mjh_mirror_create: bad argument"); return MJH_ERR_ARG; }
  mjh_mirror* m = new mjh_mirror(); m->e = e; m->env0 = env0; m->n = n;
  // (field 0, time, is one DOUBLE per env = two floats of row width: mjh_mirror_time)
  const int w[8] = {2, e->M.nq, e->M.nv, e->M.nv, 3 * e->M.nbody, 4 * e->M.nbody, 3 * e->M.ngeom, 9 * e->M.ngeom};
  for (int k = 0; k < 8; k++) { m->width[k] = w[k]; m->off[k] = m->total; m->total += (size_t)n * w[k]; }
  m->fk_floats = m->total - m->off[4];
  if (hipHostMalloc((void**)&m->host, m->total * sizeof(float), hipHostMallocDefault) != hipSuccess ||
      hipMalloc((void**)&m->dev, std::max<size_t>(m->fk_floats, 1) * sizeof(float)) != hipSuccess ||
      hipEventCreateWithFlags(&m->ev, hipEventDisableTiming) != hipSuccess) {
    mjh_set_error("mjh_mirror_create: allocation failed");
    if (m->host) (void)hipHostFree(m->host); if (m->dev) (void)hipFree(m->dev); delete m; return MJH_ERR_NO_DEVICE;
  }
  std::memset(m->host, 0, m->total * sizeof(float));
  *out = m;
  return MJH_OK;
}
extern "C" void mjh_mirror_destroy(mjh_mirror* m) {
  if (!m) return;
  (void)hipEventSynchronize(m->ev);
  (void)hipHostFree(m->host); (void)hipFree(m->dev); (void)hipEventDestroy(m->ev);
  delete m;
}
// enqueue a refresh of the selected parts (MJH_MIRROR_* bits) behind everything queued so far; returns at once
extern "C" int mjh_mirror_update(mjh_mirror* m, int what) {
  if (!m) { mjh_set_error("null mirror"); return MJH_ERR_ARG; }
  mjh_engine* e = m->e;
  ENG(e);
  const int n = m->n, env0 = m->env0;
  auto rows = [&](int k, const float* src, int stride) {
    return hipMemcpy2DAsync(m->host + m->off[k], (size_t)m->width[k] * sizeof(float), src + (size_t)env0 * stride, (size_t)stride * sizeof(float),
                            (size_t)m->width[k] * sizeof(float), (size_t)n, hipMemcpyDeviceToHost, e->stream);
  };
  if (what & MJH_MIRROR_JOINTS) {
    HIPCHK(hipMemcpyAsync(m->host + m->off[0], e->S.time + env0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, e->stream));   // time: fp64
    HIPCHK(rows(1, e->S.qpos, e->M.nqp)); HIPCHK(rows(2, e->S.qvel, e->M.nvp)); HIPCHK(rows(3, e->S.qfrc_inverse, e->M.nvp));
  }
  if (what & (MJH_MIRROR_BODIES | MJH_MIRROR_GEOMS)) {
    float* d = m->dev;
    int rc;
    {
      StateGuard guard(&e->S);
      e->S.x_xpos = d; e->S.x_xquat = d + (m->off[5] - m->off[4]); e->S.x_gpos = d + (m->off[6] - m->off[4]); e->S.x_gmat = d + (m->off[7] - m->off[4]);
      const int xf = ((what & MJH_MIRROR_BODIES) ? XF_BODY : 0) | ((what & MJH_MIRROR_GEOMS) ? XF_GEOM : 0);
      rc = launch(e, env0, n, 1, PH_FKONLY, xf);
    }
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(m->host + m->off[4], d, m->fk_floats * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  }
  HIPCHK(hipEventRecord(m->ev, e->stream));
  return MJH_OK;
}
extern "C" int mjh_mirror_wait(mjh_mirror* m) {
  if (!m) { mjh_set_error("null mirror"); return MJH_ERR_ARG; }
  HIPCHK(hipEventSynchronize(m->ev));
  return MJH_OK;
}
extern "C" const double* mjh_mirror_time(const mjh_mirror* m) { return m ? (const double*)(m->host + m->off[0]) : nullptr; }
extern "C" const float* mjh_mirror_field(const mjh_mirror* m, int which, int* row_width) {
  if (!m || which < 0 || which > 7) return nullptr;
  if (row_width) *row_width = m->width[which];
  return m->host + m->off[which];
}

extern "C" int mjh_state_stride(const mjh_engine* e) { return e ? 1 + e->M.nq + e->M.nv : 0; }
extern "C" int mjh_export_state_device(mjh_engine* e, void* d_out) {
  ENG_NOJOIN(e); if (!d_out) return MJH_ERR_ARG;
  const int stride = 1 + e->M.nq + e->M.nv;
  auto run = [&](hipStream_t st, int g0, int n) {
    const size_t total = (size_t)n * stride;
    const int blocks = (int)std::min<size_t>((total + 255) / 256, 2048);
    hipLaunchKernelGGL(mjh_export_kernel, dim3(blocks), dim3(256), 0, st, e->S, (float*)d_out, g0, n, e->M.nq, e->M.nv, e->M.nqp, e->M.nvp);
  };
  if (!e->forked) { run(e->stream, 0, e->nenv); HIPCHK(hipGetLastError()); return MJH_OK; }
  // Read-only and forked: every cohort exports its own range on its own stream, right behind its last step, and the
  // caller's stream waits for those exports only.  The cohorts stay forked, so publishing does not drain the step
  // pipeline.  (The cohort streams first wait for the caller's earlier work: it may still be reading d_out.)
  HIPCHK(hipEventRecord(e->ev_fork, e->stream));
  for (int g = 0; g < e->ncohort; g++) {
    const int g0 = (int)((long long)e->nenv * g / e->ncohort), g1 = (int)((long long)e->nenv * (g + 1) / e->ncohort);
    HIPCHK(hipStreamWaitEvent(e->cstream[g], e->ev_fork, 0));
    run(e->cstream[g], g0, g1 - g0);
    HIPCHK(hipEventRecord(e->ev_join[g], e->cstream[g]));
    HIPCHK(hipStreamWaitEvent(e->stream, e->ev_join[g], 0));
  }
  HIPCHK(hipGetLastError());
  return MJH_OK;
}

// debug: one fused step over all envs with s_memtime stamps at the 16 stage boundaries of the kernel;
// out[16] = mean over envs of (stamp[k] - stamp[0]) in shader-clock ticks
extern "C" int mjh_debug_stage_cycles(mjh_engine* e, int with_inverse, double* out) {
  ENG(e);
  DevBuf db;
  HIPCHK(hipMalloc(&db.p, (size_t)e->nenv * PROF_STRIDE * sizeof(long long)));
  long long* buf = (long long*)db.p;
  HIPCHK(hipMemsetAsync(buf, 0, (size_t)e->nenv * PROF_STRIDE * sizeof(long long), e->stream));
  int rc;
  {
    StateGuard guard(&e->S);
    e->S.x_prof = buf;
    const int ph = PH_STEP1 | PH_STEP2 | ((with_inverse & 1) ? PH_INV : 0);
    if ((with_inverse & 6) && e->M.big && e->split3) {
      // the launch chain of the many-body layout on all envs, stamps from its assemble (2) or integrate (4) launch
      const bool dn = e->M.dense != 0;
      rc = launch(e, 0, e->nenv, 1, ph | PH_PRE, (dn ? XF_DENSE : 0) | ((with_inverse & 2) ? XF_PROF : 0));
      if (!rc && dn) {
        HIPCHK(mjh_launch_dense(e->stream, e->nenv, e->dense_lds, e->dense_solve_lds, e->dC, e->S, 0));
      }
      if (!rc) {
        const size_t lds = (2 * (size_t)(((e->M.nv + 3) / 4) * 4) + 2 * (size_t)std::max(e->M.maxblk, 1) + 4 + 8 + 8 + 8 * (size_t)((e->M.nv + 2) / 3)) * sizeof(float);
        if (e->M.diagM) hipLaunchKernelGGL((mjh_solve_kernel<true, false>), dim3(e->nenv), dim3(64), lds, e->stream, e->dC, e->S, 0);
        else hipLaunchKernelGGL((mjh_solve_kernel<false, false>), dim3(e->nenv), dim3(64), lds, e->stream, e->dC, e->S, 0);
        HIPCHK(hipGetLastError());
        rc = launch(e, 0, e->nenv, 1, PH_STEP2 | PH_POST, (with_inverse & 4) ? XF_PROF : 0);
      }
    } else if ((with_inverse & 8) && e->M.window && e->S.wbuf) {
      // the window chain's assemble-only instance alone, every env handed over (no window launch: the guard puts the state back)
      rc = launch(e, 0, e->nenv, 1, ph, XF_PROF, 1);
    } else
    rc = launch(e, 0, e->nenv, 1, ph, XF_PROF);
  }
  std::vector<long long> h((size_t)e->nenv * PROF_STRIDE);
  if (!rc) { HIPCHK(hipMemcpyAsync(h.data(), buf, h.size() * sizeof(long long), hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream)); }
  if (rc) return rc;
  for (int k = 0; k < 16; k++) out[k] = 0;
  for (int en = 0; en < e->nenv; en++) for (int k = 0; k < 16; k++) { long long v = h[(size_t)en*PROF_STRIDE+k]; out[k] += v ? (double)(v - h[(size_t)en*PROF_STRIDE]) : 0.0; }
  for (int k = 0; k < 16; k++) out[k] /= e->nenv;
#ifdef MJH_COLLIDE_PROBE
  // probe build: out[16 .. 18] the three stamps inside the collision stage (the caller passes 20 doubles)
  for (int k = 0; k < 3; k++) {
    out[16 + k] = 0;
    for (int en = 0; en < e->nenv; en++) { long long v = h[(size_t)en*PROF_STRIDE+20+k]; out[16 + k] += v ? (double)(v - h[(size_t)en*PROF_STRIDE]) : 0.0; }
    out[16 + k] /= e->nenv;
  }
#endif
  return MJH_OK;
}

// Debug: the solve launch of the many-body chain (free-body models: C2) on the pools the last step left, timed with HIP events —
// once as it is, once with every wave reading the block operands of one of `slices` environments (a working set that stays in L2):
// the difference is what the operand stream from MALL / HBM costs.  out_ms[2], out_iter[2] (mean sweeps).  The probe's results are
// garbage: the next step rebuilds the pools; state, clock and warm start are not touched (the launches write qacc only into the
// chain's hand-over slice).
extern "C" int mjh_debug_solve_probe(mjh_engine* e, int slices, int reps, double* out_ms, double* out_iter) {
  ENG(e);
  if (!(e->M.big && e->split3 && e->M.diagM)) { mjh_set_error("mjh_debug_solve_probe: free-body model in the many-body layout only"); return MJH_ERR_ARG; }
  hipEvent_t a, b; HIPCHK(hipEventCreate(&a)); HIPCHK(hipEventCreate(&b));
  const size_t lds = (2 * (size_t)(((e->M.nv + 3) / 4) * 4) + 2 * (size_t)std::max(e->M.maxblk, 1) + 4 + 8 + 8 + 8 * (size_t)((e->M.nv + 2) / 3)) * sizeof(float);
  std::vector<float> meta((size_t)e->nenv);
  for (int mode = 0; mode < 2; mode++) {
    StateGuard guard(&e->S);
    e->S.probe_slices = mode ? std::max(1, slices) : 0; e->S.env_order = nullptr;
    HIPCHK(hipEventRecord(a, e->stream));
    for (int r = 0; r < std::max(1, reps); r++) hipLaunchKernelGGL((mjh_solve_kernel<true, false>), dim3(e->nenv), dim3(64), lds, e->stream, e->dC, e->S, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(b, e->stream)); HIPCHK(hipEventSynchronize(b));
    float ms = 0; HIPCHK(hipEventElapsedTime(&ms, a, b)); out_ms[mode] = ms / std::max(1, reps);
    double it = 0;
    HIPCHK(hipMemcpy2D(meta.data(), sizeof(float), e->S.gscratch + e->L.g_meta + 5, (size_t)e->S.gstride * sizeof(float), sizeof(float), (size_t)e->nenv, hipMemcpyDeviceToHost));
    for (int i = 0; i < e->nenv; i++) { int v; std::memcpy(&v, &meta[i], 4); it += v; }
    out_iter[mode] = it / e->nenv;
  }
  (void)hipEventDestroy(a); (void)hipEventDestroy(b);
  return MJH_OK;
}

// raw per-env stamps of one LPT-ordered step launch (debug timeline tool): out[nenv*PROF_STRIDE]
extern "C" int mjh_debug_stage_raw(mjh_engine* e, int with_inverse, long long* out) {
  ENG(e);
  DevBuf db;
  HIPCHK(hipMalloc(&db.p, (size_t)e->nenv * PROF_STRIDE * sizeof(long long)));
  long long* buf = (long long*)db.p;
  HIPCHK(hipMemsetAsync(buf, 0, (size_t)e->nenv * PROF_STRIDE * sizeof(long long), e->stream));
  int rc;
  {
    StateGuard guard(&e->S);
    e->S.x_prof = buf;
    if (e->lpt && e->d_order) {
      hipLaunchKernelGGL(mjh_order_kernel, dim3(1), dim3(1024), 0, e->stream, (const int*)e->S.stats, e->d_order, 0, e->nenv, (int*)nullptr, 0);
      e->S.env_order = e->d_order; e->order_valid = true; e->order_G = -1;
    }
    rc = launch(e, 0, e->nenv, 1, PH_STEP1 | PH_STEP2 | (with_inverse ? PH_INV : 0), XF_PROF);
  }
  if (!rc) { HIPCHK(hipMemcpyAsync(out, buf, (size_t)e->nenv * PROF_STRIDE * sizeof(long long), hipMemcpyDeviceToHost, e->stream)); HIPCHK(hipStreamSynchronize(e->stream)); }
  return rc;
}

// debug: one full-range step launch that returns at stage boundary `stage` (1..14) without storing anything
extern "C" int mjh_debug_stop_at(mjh_engine* e, int stage, int with_inverse) {
  ENG(e);
  if (stage < 1 || stage > 14) { mjh_set_error("mjh_debug_stop_at: stage must be 1..14"); return MJH_ERR_ARG; }
  return launch(e, 0, e->nenv, 1, PH_STEP1 | PH_STEP2 | (with_inverse ? PH_INV : 0), stage << 8);
}

// ---- batched ray casting (mj_ray for every env: laser scans, range finders, terrain height under a foot) and depth images
// what a ray can see of geom g in mesh mode 0: its type, or -1 (mesh geoms; an hfield geom without an asset)
static int ray_geom_type(const mjh_model* m, int g) {
  const int t = m->geom_type[g];
  if (t == MJH_GEOM_MESH) return -1;
  if (t == MJH_GEOM_HFIELD && !(m->nhfield > 0 && m->geom_dataid && m->geom_dataid[g] >= 0 && m->geom_dataid[g] < m->nhfield)) return -1;
  return t < MJH_GEOM_PLANE || t > MJH_GEOM_BOX ? -1 : t;
}
extern "C" int mjh_ray_skipped_geoms(const mjh_model* m) {
  if (!m) return 0;
  int n = 0;
  for (int g = 0; g < m->ngeom; g++) n += ray_geom_type(m, g) < 0;
  return n;
}
extern "C" void mjh_ray_default_options(mjh_ray_options* o) {
  if (!o) return;
  o->site = -1; o->bodyexclude = -1; o->flg_static = 1; o->per_env = 0; o->cutoff = 0.0;
}
static int ray_tables(mjh_engine* e) {
  if (e->ray_ready) return MJH_OK;
  const mjh_model* m = e->model;
  std::vector<int4> gi((size_t)std::max(m->ngeom, 1));
  for (int g = 0; g < m->ngeom; g++) {
    const int t = ray_geom_type(m, g), b = m->geom_bodyid[g];
    gi[g] = make_int4(t, b, m->body_weldid[b] == 0 ? 1 : 0, t == MJH_GEOM_HFIELD ? m->geom_dataid[g] : -1);
  }
  int rc = dev_alloc(e, &e->ray_ginfo, gi.size(), false);
  if (rc) return rc;
  HIPCHK(hipMemcpy(e->ray_ginfo, gi.data(), gi.size() * sizeof(int4), hipMemcpyHostToDevice));
  if (m->nhfield > 0) {
    std::vector<RayHField> hf((size_t)m->nhfield);
    std::vector<float> hd((size_t)std::max(m->nhfielddata, 1));
    for (int h = 0; h < m->nhfield; h++) {
      hf[h].nrow = m->hfield_nrow[h]; hf[h].ncol = m->hfield_ncol[h]; hf[h].adr = m->hfield_adr[h]; hf[h].pad = 0;
      for (int k = 0; k < 4; k++) hf[h].size[k] = (float)m->hfield_size[4*h + k];
    }
    for (int i = 0; i < m->nhfielddata; i++) hd[i] = (float)m->hfield_data[i];
    rc = dev_alloc(e, &e->ray_hf, hf.size(), false);
    if (!rc) rc = dev_alloc(e, &e->ray_hfdata, hd.size(), false);
    if (rc) return rc;
    HIPCHK(hipMemcpy(e->ray_hf, hf.data(), hf.size() * sizeof(RayHField), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(e->ray_hfdata, hd.data(), hd.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  e->ray_ginfo_mesh = e->ray_ginfo;
  if (m->nmesh > 0 && m->nmeshplane > 0 && m->mesh_plane && m->mesh_planeadr && m->mesh_planenum && m->geom_dataid) {
    // mode 1: a mesh geom whose asset has hull planes is typed MJH_GEOM_MESH, w = its mesh id (a mesh without volume stays invisible)
    // (every mesh's planes padded to a multiple of four with planes that clip nothing: dev_ray.h, ray_convex)
    std::vector<RayMesh> mt((size_t)m->nmesh);
    std::vector<float4> pl;
    pl.reserve((size_t)m->nmeshplane + 3 * (size_t)m->nmesh);
    for (int i = 0; i < m->nmesh; i++) {
      const int adr = m->mesh_planeadr[i], num = m->mesh_planenum[i];
      const bool ok = adr >= 0 && num > 0 && (long long)adr + num <= m->nmeshplane;
      double r2 = 0;
      for (int k = 0; k < m->mesh_vertnum[i]; k++) { const double* x = m->mesh_vert + 3 * ((size_t)m->mesh_vertadr[i] + k); r2 = std::max(r2, x[0]*x[0] + x[1]*x[1] + x[2]*x[2]); }
      ray_append_planes(m->mesh_plane + 4 * (size_t)(ok ? adr : 0), ok ? num : 0, (float)std::sqrt(r2), pl, mt[i]);
    }
    if (pl.empty()) pl.push_back(make_float4(0.0f, 0.0f, 0.0f, 1.0f));
    bool any = false;
    for (int g = 0; g < m->ngeom; g++) {
      const int id = m->geom_dataid[g];
      if (m->geom_type[g] == MJH_GEOM_MESH && id >= 0 && id < m->nmesh && mt[id].num > 0) { gi[g].x = MJH_GEOM_MESH; gi[g].w = id; any = true; }
    }
    if (any) {
      rc = dev_alloc(e, &e->ray_ginfo_mesh, gi.size(), false);
      if (!rc) rc = dev_alloc(e, &e->ray_mesh, mt.size(), false);
      if (!rc) rc = dev_alloc(e, &e->ray_planes, pl.size(), false);
      if (rc) return rc;
      HIPCHK(hipMemcpy(e->ray_ginfo_mesh, gi.data(), gi.size() * sizeof(int4), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->ray_mesh, mt.data(), mt.size() * sizeof(RayMesh), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(e->ray_planes, pl.data(), pl.size() * sizeof(float4), hipMemcpyHostToDevice));
    }
  }
  e->ray_gi_mesh_host = gi;
  e->ray_ready = true;
  return MJH_OK;
}
// the tables of mesh surface 1 (after ray_tables): a BVH per mesh asset with triangles (ray_bvh.h), all of them in one node and one
// triangle array, and the geom table that types those assets' geoms RAY_TYPE_TRIMESH — a mesh geom without triangles keeps its row of the
// mode-1 table (its hull, or invisible)
static int ray_tri_tables(mjh_engine* e) {
  if (e->ray_tri_ready) return MJH_OK;
  const mjh_model* m = e->model;
  e->ray_ginfo_tri = e->ray_ginfo_mesh;
  if (m->nmesh > 0 && m->nmeshtri > 0 && m->mesh_tri && m->mesh_triadr && m->mesh_trinum && m->geom_dataid) {
    std::vector<RayTriMesh> mt((size_t)m->nmesh, RayTriMesh{0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f});
    std::vector<RayNode> nodes; std::vector<float> tris;
    for (int i = 0; i < m->nmesh; i++) {
      const int adr = m->mesh_triadr[i], num = m->mesh_trinum[i];
      if (!(adr >= 0 && num > 0 && (long long)adr + num <= m->nmeshtri)) continue;
      const int bad = ray_append_bvh(m->mesh_tri + 9 * (size_t)adr, num, nodes, tris, mt[i]);
      if (bad == RAY_APPEND_NO_BVH) { mjh_set_error("mjh_ray: the triangles of mesh " + std::to_string(i) + " give no valid BVH (non-finite coordinates?)"); return MJH_ERR_ARG; }
      if (bad) { mjh_set_error("mjh_ray: too many mesh triangles"); return MJH_ERR_ARG; }
    }
    std::vector<int4> gi = e->ray_gi_mesh_host;
    bool any = false;
    for (int g = 0; g < m->ngeom; g++) {
      const int id = m->geom_dataid[g];
      if (m->geom_type[g] == MJH_GEOM_MESH && id >= 0 && id < m->nmesh && mt[id].nnode > 0) { gi[g].x = RAY_TYPE_TRIMESH; gi[g].w = id; any = true; }
    }
    if (any) {
      // (the engine's pointers are set once all four tables are filled: a failed allocation or copy leaves the hull's table in place)
      int4* d_gi = nullptr; RayTriMesh* d_mt = nullptr; RayNode* d_nodes = nullptr; float4* d_tris = nullptr;
      int rc = dev_alloc(e, &d_gi, gi.size(), false);
      if (!rc) rc = dev_alloc(e, &d_mt, mt.size(), false);
      if (!rc) rc = dev_alloc(e, &d_nodes, nodes.size(), false);
      if (!rc) rc = dev_alloc(e, &d_tris, tris.size() / 4, false);
      if (rc) return rc;
      HIPCHK(hipMemcpy(d_gi, gi.data(), gi.size() * sizeof(int4), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_mt, mt.data(), mt.size() * sizeof(RayTriMesh), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_nodes, nodes.data(), nodes.size() * sizeof(RayNode), hipMemcpyHostToDevice));
      HIPCHK(hipMemcpy(d_tris, tris.data(), tris.size() * sizeof(float), hipMemcpyHostToDevice));
      e->ray_ginfo_tri = d_gi; e->ray_trimesh = d_mt; e->ray_nodes = d_nodes; e->ray_tris = d_tris;
    }
  }
  e->ray_tri_ready = true;
  return MJH_OK;
}
extern "C" int mjh_ray_set_mesh_surface(mjh_engine* e, int surface) {
  ENG(e);
  if (surface != MJH_RAY_SURFACE_HULL && surface != MJH_RAY_SURFACE_TRIANGLES) { mjh_set_error("mjh_ray_set_mesh_surface: surface must be 0 (hull) or 1 (triangles)"); return MJH_ERR_ARG; }
  e->ray_mesh_surface = surface;      // (the next ray launch takes the surface's geom table by value; the triangle tables are built by that launch)
  return MJH_OK;
}
extern "C" int mjh_ray_get_mesh_surface(const mjh_engine* e) { return e ? e->ray_mesh_surface : 0; }
extern "C" int mjh_ray_set_mesh_mode(mjh_engine* e, int mode) {
  ENG(e);
  if (mode != 0 && mode != 1) { mjh_set_error("mjh_ray_set_mesh_mode: mode must be 0 or 1"); return MJH_ERR_ARG; }
  e->ray_mesh_mode = mode;      // (both geom tables are resident: the next ray launch takes the mode's own by value)
  return MJH_OK;
}
extern "C" int mjh_ray_get_mesh_mode(const mjh_engine* e) { return e ? e->ray_mesh_mode : 0; }
// argument checks shared by both entry points: nothing is launched when one fails
static int ray_check(const mjh_engine* e, int env0, int n, int nray, const void* pnt, const void* vec, const mjh_ray_options* o, const void* dist, const void* geomid) {
  if (env0 < 0 || n <= 0 || env0 + n > e->nenv) { mjh_set_error("mjh_ray: env range out of bounds"); return MJH_ERR_ARG; }
  if (nray <= 0 || (long long)nray * n > 0x3fffffffLL) { mjh_set_error("mjh_ray: nray must be positive (and n * nray below 2^30)"); return MJH_ERR_ARG; }
  if (!pnt || !vec || !dist || !geomid) { mjh_set_error("mjh_ray: null pointer"); return MJH_ERR_ARG; }
  if (o) {
    if (o->site < -1 || o->site >= e->model->nsite) { mjh_set_error("mjh_ray: site id out of range"); return MJH_ERR_ARG; }
    if (o->bodyexclude < -1 || o->bodyexclude >= e->model->nbody) { mjh_set_error("mjh_ray: bodyexclude out of range"); return MJH_ERR_ARG; }
  }
  return MJH_OK;
}
// The launch chain of mjh_ray_device and mjh_depth_device: the position-stage launch of the env range (PH_FKONLY with XF_GEOM, plus
// XF_BODY when `bodies`: a site's or a camera's frame) into the engine's export scratch, exactly as fk_export issues it; the caller's
// kernel follows on the same stream and reads what *W (and, with mesh surface 1, *T) names.  Nothing of the envs' state, statistics or time is written.
static int ray_scene(mjh_engine* e, int env0, int n, bool bodies, int bodyexclude, int flg_static, double cutoff, RayScene* W, RayTris* T) {
  int rc = ray_tables(e);
  if (!rc && e->ray_mesh_surface == MJH_RAY_SURFACE_TRIANGLES) rc = ray_tri_tables(e);
  if (rc) return rc;
  const int ng = e->M.ngeom, nb = e->M.nbody;
  const size_t fg = (size_t)n * 3 * ng, fm = (size_t)n * 9 * ng, fx = bodies ? (size_t)n * 3 * nb : 0, fq = bodies ? (size_t)n * 4 * nb : 0;
  rc = ensure_scratch(e, fg + fm + fx + fq);
  if (rc) return rc;
  W->gpos = e->scratch; W->gmat = e->scratch + fg;
  W->xpos = bodies ? e->scratch + fg + fm : nullptr; W->xquat = bodies ? e->scratch + fg + fm + fx : nullptr;
  {
    StateGuard guard(&e->S);
    e->S.x_gpos = e->scratch; e->S.x_gmat = e->scratch + fg;
    if (bodies) { e->S.x_xpos = e->scratch + fg + fm; e->S.x_xquat = e->scratch + fg + fm + fx; }
    rc = launch(e, env0, n, 1, PH_FKONLY, XF_GEOM | (bodies ? XF_BODY : 0));
  }
  if (rc) return rc;
  if (e->S.p_geom_size) { W->size = e->S.p_geom_size; W->size_stride = e->S.p_stride; } else { W->size = e->dF + e->M.o_geom_size; W->size_stride = 0; }
  W->slot_mask = e->S.slot_mask; W->sbase = nb > 32 ? nb - 32 : 0;
  const bool tri = e->ray_mesh_mode && e->ray_mesh_surface == MJH_RAY_SURFACE_TRIANGLES;
  W->ginfo = !e->ray_mesh_mode ? e->ray_ginfo : (tri ? e->ray_ginfo_tri : e->ray_ginfo_mesh); W->hf = e->ray_hf; W->hf_data = e->ray_hfdata;
  W->mesh = e->ray_mesh; W->planes = e->ray_planes;
  T->mesh = tri ? e->ray_trimesh : nullptr; T->nodes = tri ? e->ray_nodes : nullptr; T->tris = tri ? e->ray_tris : nullptr;
  W->env0 = env0; W->n = n; W->ngeom = ng; W->nbody = nb;
  W->bodyexclude = bodyexclude; W->flg_static = flg_static ? 1 : 0; W->cutoff = cutoff > 0 ? (float)cutoff : 0.0f;
  return MJH_OK;
}
// an engine-owned device buffer grown to `need` floats (the stream is drained before a buffer it may still use is freed)
static int io_reserve(mjh_engine* e, float** buf, size_t* have, size_t need) {
  if (need <= *have) return MJH_OK;
  if (*buf) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(*buf)); *buf = nullptr; *have = 0; }
  HIPCHK(hipMalloc((void**)buf, need * sizeof(float)));
  *have = need;
  return MJH_OK;
}
// the device staging buffer of mjh_ray, mjh_depth and mjh_render
static int ray_io_reserve(mjh_engine* e, size_t need) { return io_reserve(e, &e->ray_io, &e->ray_io_floats, need); }
// a site's frame in its body for a launch descriptor (RayArgs, ScanArgs, HScanArgs); site < 0: the world frame
template <class Args>
static void site_frame(const mjh_model* m, int site, Args* A) {
  A->site_body = -1;
  if (site < 0) return;
  A->site_body = m->site_bodyid[site];
  for (int k = 0; k < 3; k++) A->site_pos[k] = (float)m->site_pos[3 * site + k];
  for (int k = 0; k < 4; k++) A->site_quat[k] = (float)m->site_quat[4 * site + k];
}
// the host form of a scan (mjh_scan, mjh_heightscan): range, geom id and points of `nout` beams carved out of the staging buffer,
// device(d_range, d_geomid, d_points) with null where the caller takes none, then read back in stream order
template <class Device>
static int scan_readback(mjh_engine* e, size_t nout, float* range, int* geomid, float* points, Device device) {
  int rc = ray_io_reserve(e, 5 * nout);
  if (rc) return rc;
  float* const d_range = e->ray_io; int* const d_gid = (int*)(e->ray_io + nout); float* const d_pts = e->ray_io + 2 * nout;
  rc = device(d_range, geomid ? d_gid : nullptr, points ? d_pts : nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(range, d_range, nout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (geomid) HIPCHK(hipMemcpyAsync(geomid, d_gid, nout * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (points) HIPCHK(hipMemcpyAsync(points, d_pts, 3 * nout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}
extern "C" int mjh_ray_device(mjh_engine* e, int env0, int n, int nray, const float* d_pnt, const float* d_vec, const mjh_ray_options* opt,
                              float* d_dist, int* d_geomid) {
  ENG(e);
  int rc = ray_check(e, env0, n, nray, d_pnt, d_vec, opt, d_dist, d_geomid);
  if (rc) return rc;
  mjh_ray_options o; mjh_ray_default_options(&o);
  if (opt) o = *opt;
  RayArgs A{};
  rc = ray_scene(e, env0, n, o.site >= 0, o.bodyexclude, o.flg_static, o.cutoff, &A.W, &A.T);
  if (rc) return rc;
  A.pnt = d_pnt; A.vec = d_vec; A.dist = d_dist; A.geomid = d_geomid;
  A.nray = nray; A.per_env = o.per_env ? 1 : 0;
  site_frame(e->model, o.site, &A);
  HIPCHK(mjh_launch_ray(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_ray(mjh_engine* e, int env0, int n, int nray, const double* pnt, const double* vec, const mjh_ray_options* opt,
                       double* dist, int* geomid) {
  ENG(e);
  int rc = ray_check(e, env0, n, nray, pnt, vec, opt, dist, geomid);
  if (rc) return rc;
  const size_t nin = (size_t)(opt && opt->per_env ? n : 1) * nray, nout = (size_t)n * nray;
  std::vector<float> h(6 * nin);
  for (size_t i = 0; i < nin; i++) {
    if (vec[3*i] == 0.0 && vec[3*i+1] == 0.0 && vec[3*i+2] == 0.0) { mjh_set_error("mjh_ray: zero direction vector"); return MJH_ERR_ARG; }
    for (int k = 0; k < 3; k++) { h[3*i + k] = (float)pnt[3*i + k]; h[3*nin + 3*i + k] = (float)vec[3*i + k]; }
  }
  rc = ray_io_reserve(e, 6 * nin + 2 * nout);
  if (rc) return rc;
  float* const d_in = e->ray_io; float* const d_dist = e->ray_io + 6 * nin; int* const d_gid = (int*)(e->ray_io + 6 * nin + nout);
  HIPCHK(hipMemcpyAsync(d_in, h.data(), 6 * nin * sizeof(float), hipMemcpyHostToDevice, e->stream));
  rc = mjh_ray_device(e, env0, n, nray, d_in, d_in + 3 * nin, opt, d_dist, d_gid);
  if (rc) { (void)hipStreamSynchronize(e->stream); return rc; }      // (the upload reads `h`)
  std::vector<float> hd(nout);
  HIPCHK(hipMemcpyAsync(hd.data(), d_dist, nout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(geomid, d_gid, nout * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < nout; i++) dist[i] = (double)hd[i];
  return MJH_OK;
}

// ---- depth images (mjh_depth / mjh_depth_device, depth.hip): ray_scene() with the body poses, then mjh_depth_kernel on the same stream.
// The camera's world pose is formed on the device from its body's exported pose.
extern "C" void mjh_depth_default_options(mjh_depth_options* o) {
  if (!o) return;
  o->camera = 0; o->width = 64; o->height = 64; o->bodyexclude = -1; o->flg_static = 1; o->range = 0; o->cull = 1; o->cutoff = 0.0;
}
// argument checks shared by both entry points: nothing is launched when one fails
static int depth_check(const mjh_engine* e, int env0, int n, const mjh_depth_options& o, const void* depth, bool need_depth = true) {
  const mjh_model* m = e->model;
  if (m->ncam <= 0) { mjh_set_error("mjh_depth: the model has no camera"); return MJH_ERR_ARG; }
  if (o.camera < 0 || o.camera >= m->ncam) { mjh_set_error("mjh_depth: camera id out of range"); return MJH_ERR_ARG; }
  if (o.bodyexclude < -1 || o.bodyexclude >= m->nbody) { mjh_set_error("mjh_depth: bodyexclude out of range"); return MJH_ERR_ARG; }
  if (env0 < 0 || n <= 0 || env0 + n > e->nenv) { mjh_set_error("mjh_depth: env range out of bounds"); return MJH_ERR_ARG; }
  if (o.width <= 0 || o.height <= 0 || (long long)o.width * o.height * n > 0x3fffffffLL) { mjh_set_error("mjh_depth: width and height must be positive (and n * width * height below 2^30)"); return MJH_ERR_ARG; }
  if (need_depth && !depth) { mjh_set_error("mjh_depth: null pointer"); return MJH_ERR_ARG; }
  return MJH_OK;
}
// ray_scene() and the depth launch's descriptor (checked options): what mjh_depth_device and mjh_render_device hand to mjh_launch_depth
static int depth_chain(mjh_engine* e, int env0, int n, const mjh_depth_options& o, float* d_depth, int* d_geomid, DepthArgs* A) {
  const mjh_model* m = e->model;
  int rc = ray_scene(e, env0, n, true, o.bodyexclude, o.flg_static, o.cutoff, &A->W, &A->T);
  if (rc) return rc;
  A->depth = d_depth; A->geomid = d_geomid;
  A->width = o.width; A->height = o.height; A->range = o.range ? 1 : 0; A->cull = o.cull ? 1 : 0;
  A->cam_body = m->cam_bodyid[o.camera];
  for (int k = 0; k < 3; k++) A->cam_pos[k] = (float)m->cam_pos[3 * o.camera + k];
  for (int k = 0; k < 4; k++) A->cam_quat[k] = (float)m->cam_quat[4 * o.camera + k];
  A->scale = (float)(std::tan(0.5 * m->cam_fovy[o.camera] * 3.14159265358979323846 / 180.0) / (double)o.height);
  return MJH_OK;
}
extern "C" int mjh_depth_device(mjh_engine* e, int env0, int n, const mjh_depth_options* opt, float* d_depth, int* d_geomid) {
  ENG(e);
  mjh_depth_options o; mjh_depth_default_options(&o);
  if (opt) o = *opt;
  int rc = depth_check(e, env0, n, o, d_depth);
  if (rc) return rc;
  DepthArgs A{};
  rc = depth_chain(e, env0, n, o, d_depth, d_geomid, &A);
  if (rc) return rc;
  HIPCHK(mjh_launch_depth(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_depth(mjh_engine* e, int env0, int n, const mjh_depth_options* opt, float* depth, int* geomid) {
  ENG(e);
  mjh_depth_options o; mjh_depth_default_options(&o);
  if (opt) o = *opt;
  int rc = depth_check(e, env0, n, o, depth);
  if (rc) return rc;
  const size_t nout = (size_t)n * o.width * o.height;
  rc = ray_io_reserve(e, 2 * nout);
  if (rc) return rc;
  float* const d_depth = e->ray_io; int* const d_gid = (int*)(e->ray_io + nout);
  rc = mjh_depth_device(e, env0, n, &o, d_depth, geomid ? d_gid : nullptr);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(depth, d_depth, nout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (geomid) HIPCHK(hipMemcpyAsync(geomid, d_gid, nout * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}

// ---- lidar range images (mjh_scan / mjh_scan_device, scan.hip): the pattern's angle tables (dev_scan.h) on the engine's stream when the
// pattern is not the last call's, ray_scene() (with the body poses when the sensor is a site), then mjh_scan_kernel on the same stream.
extern "C" void mjh_scan_default_options(mjh_scan_options* o) {
  if (!o) return;
  o->site = -1; o->width = 360; o->height = 1;
  o->azimuth0 = -3.14159265358979323846; o->azimuth_step = 2.0 * 3.14159265358979323846 / 360.0;
  o->elevation = nullptr; o->elevation0 = 0.0; o->elevation_step = 0.0;
  o->bodyexclude = -1; o->flg_static = 1; o->cull = 1; o->cutoff = 0.0;
}
// argument checks shared by both entry points: nothing is launched when one fails
static int scan_check(const mjh_engine* e, int env0, int n, const mjh_scan_options& o, const void* range) {
  const mjh_model* m = e->model;
  if (o.site < -1 || o.site >= m->nsite) { mjh_set_error("mjh_scan: site id out of range"); return MJH_ERR_ARG; }
  if (o.bodyexclude < -1 || o.bodyexclude >= m->nbody) { mjh_set_error("mjh_scan: bodyexclude out of range"); return MJH_ERR_ARG; }
  if (env0 < 0 || n <= 0 || env0 + n > e->nenv) { mjh_set_error("mjh_scan: env range out of bounds"); return MJH_ERR_ARG; }
  if (const char* bad = scan_pattern_error(o.width, o.height, n, o.azimuth0, o.azimuth_step, o.elevation, o.elevation0, o.elevation_step)) {
    mjh_set_error(std::string("mjh_scan: ") + bad); return MJH_ERR_ARG;
  }
  if (!range) { mjh_set_error("mjh_scan: null pointer"); return MJH_ERR_ARG; }
  return MJH_OK;
}
// the tables of the (checked) pattern in e->scan_tab: uploaded in stream order from the engine's pinned buffer unless they are there already
static int scan_tables(mjh_engine* e, const mjh_scan_options& o) {
  const bool table = o.elevation != nullptr;
  bool same = e->scan_have && e->scan_w == o.width && e->scan_h == o.height && e->scan_az[0] == o.azimuth0 && e->scan_az[1] == o.azimuth_step && e->scan_table == table;
  if (same && table) same = std::equal(e->scan_elev.begin(), e->scan_elev.end(), o.elevation);
  if (same && !table) same = e->scan_el[0] == o.elevation0 && e->scan_el[1] == o.elevation_step;
  if (same) return MJH_OK;
  e->scan_have = false;
  const size_t need = 2 * ((size_t)o.width + (size_t)o.height);
  if (!e->scan_up) HIPCHK(hipEventCreateWithFlags(&e->scan_up, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(e->scan_up));      // (the last upload has read the host buffer)
  if (need > e->scan_host_floats) {
    if (e->scan_host) { HIPCHK(hipHostFree(e->scan_host)); e->scan_host = nullptr; e->scan_host_floats = 0; }
    HIPCHK(hipHostMalloc((void**)&e->scan_host, need * sizeof(float), hipHostMallocDefault));
    e->scan_host_floats = need;
  }
  int rc = io_reserve(e, &e->scan_tab, &e->scan_tab_floats, need);
  if (rc) return rc;
  scan_fill_tables(o.width, o.height, o.azimuth0, o.azimuth_step, o.elevation, o.elevation0, o.elevation_step, e->scan_host);
  HIPCHK(hipMemcpyAsync(e->scan_tab, e->scan_host, need * sizeof(float), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipEventRecord(e->scan_up, e->stream));
  e->scan_w = o.width; e->scan_h = o.height; e->scan_az[0] = o.azimuth0; e->scan_az[1] = o.azimuth_step;
  e->scan_table = table; e->scan_el[0] = o.elevation0; e->scan_el[1] = o.elevation_step;
  if (table) e->scan_elev.assign(o.elevation, o.elevation + o.height); else e->scan_elev.clear();
  e->scan_have = true;
  return MJH_OK;
}
extern "C" int mjh_scan_device(mjh_engine* e, int env0, int n, const mjh_scan_options* opt, float* d_range, int* d_geomid, float* d_points) {
  ENG(e);
  mjh_scan_options o; mjh_scan_default_options(&o);
  if (opt) o = *opt;
  int rc = scan_check(e, env0, n, o, d_range);
  if (rc) return rc;
  rc = scan_tables(e, o);
  if (rc) return rc;
  ScanArgs A{};
  rc = ray_scene(e, env0, n, o.site >= 0, o.bodyexclude, o.flg_static, o.cutoff, &A.W, &A.T);
  if (rc) return rc;
  A.range = d_range; A.geomid = d_geomid; A.points = d_points; A.tab = e->scan_tab;
  A.width = o.width; A.height = o.height; A.tw_log = scan_tile_shape(o.height); A.cull = o.cull ? 1 : 0;
  A.az_step = (float)std::fabs(o.azimuth_step);
  if (!(A.az_step >= std::fabs(o.azimuth_step))) A.az_step = std::nextafter(A.az_step, INFINITY);      // (rounded up: the half-span test may only err towards `no cone`)
  site_frame(e->model, o.site, &A);
  HIPCHK(mjh_launch_scan(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_scan(mjh_engine* e, int env0, int n, const mjh_scan_options* opt, float* range, int* geomid, float* points) {
  ENG(e);
  mjh_scan_options o; mjh_scan_default_options(&o);
  if (opt) o = *opt;
  int rc = scan_check(e, env0, n, o, range);
  if (rc) return rc;
  return scan_readback(e, (size_t)n * o.width * o.height, range, geomid, points,
                       [&](float* d_range, int* d_geomid, float* d_points) { return mjh_scan_device(e, env0, n, &o, d_range, d_geomid, d_points); });
}

// ---- contact report (mjh_set_contact_report): the readers of what the step kernel's report stage left (step_kernel.h), and the per-body
// contact force (contact.hip) on the same stream.
static_assert(CF_REC_WORDS == CREP_STRIDE && CF_FORCE == CREP_FORCE && CF_GEOM1 == CREP_GEOM1 && CF_GEOM2 == CREP_GEOM2, "contact.hip reads the step kernel's record");
extern "C" int mjh_contact_report(const mjh_engine* e) { return e ? (e->report ? 1 : 0) : g_contact_report; }      // (NULL: the switch itself)
#define REPORT_ON(e, who) if (!(e)->report) { mjh_set_error(std::string(who) + ": the engine was created with the contact report off (mjh_set_contact_report)"); return MJH_ERR_STATE; }
extern "C" int mjh_contact_report_device(mjh_engine* e, const void** d_ncon, const void** d_records, const void** d_cfrc_ext, int* maxcon) {
  ENG_NOJOIN(e); KEEP_HANDOVER(e);
  REPORT_ON(e, "mjh_contact_report_device");
  if (d_ncon) *d_ncon = e->R.ncon;
  if (d_records) *d_records = e->R.rec;
  if (d_cfrc_ext) *d_cfrc_ext = e->R.cfrc;
  if (maxcon) *maxcon = e->R.maxcon;
  return MJH_OK;
}
extern "C" int mjh_get_contact_forces(mjh_engine* e, int env0, int n, int* ncon, double* dist, double* pos, double* frame, double* force, int* geom, int* dim) {
  ENG(e); KEEP_HANDOVER(e);
  REPORT_ON(e, "mjh_get_contact_forces");
  RANGE(e, env0, n);
  if (n == 0) return MJH_OK;
  const int mc = e->R.maxcon;
  std::vector<int> nc((size_t)n);
  std::vector<float> rec((size_t)n * mc * CREP_STRIDE);
  HIPCHK(hipMemcpyAsync(nc.data(), e->R.ncon + env0, nc.size() * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipMemcpyAsync(rec.data(), e->R.rec + (size_t)env0 * mc * CREP_STRIDE, rec.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < n; i++) {
    const int k = std::max(0, std::min(nc[i], mc));
    if (ncon) ncon[i] = k;
    for (int c = 0; c < mc; c++) {
      const size_t o = (size_t)i * mc + c;
      const float* r = rec.data() + o * CREP_STRIDE;
      const bool live = c < k;
      if (dist) dist[o] = live ? r[0] : 0.0;
      if (pos) for (int q = 0; q < 3; q++) pos[3*o+q] = live ? r[1+q] : 0.0;
      if (frame) for (int q = 0; q < 9; q++) frame[9*o+q] = live ? r[4+q] : 0.0;
      if (force) for (int q = 0; q < 6; q++) force[6*o+q] = (live && q < 4) ? r[CREP_FORCE+q] : 0.0;
      int g[3] = {0, 0, 0};
      if (live) std::memcpy(g, r + CREP_GEOM1, sizeof g);
      if (geom) { geom[2*o] = g[0]; geom[2*o+1] = g[1]; }
      if (dim) dim[o] = g[2];
    }
  }
  return MJH_OK;
}
extern "C" int mjh_get_cfrc_ext(mjh_engine* e, int env0, int n, double* cfrc_ext) {
  ENG(e); KEEP_HANDOVER(e);
  REPORT_ON(e, "mjh_get_cfrc_ext");
  RANGE(e, env0, n);
  if (!cfrc_ext) return MJH_ERR_ARG;
  const int w = 6 * e->M.nbody;
  return get_rows(e, e->R.cfrc, w, w, env0, n, cfrc_ext);
}
// argument checks shared by both entry points: nothing is launched when one fails
static int body_force_check(const mjh_engine* e, int env0, int n, int nsel, const int* body, const int* against, const void* force) {
  if (env0 < 0 || n <= 0 || env0 + n > e->nenv) { mjh_set_error("mjh_body_contact_force: env range out of bounds"); return MJH_ERR_ARG; }
  if (nsel <= 0 || !body || !force) { mjh_set_error("mjh_body_contact_force: empty selection or null pointer"); return MJH_ERR_ARG; }
  if ((long long)n * nsel >= (1ll << 30)) { mjh_set_error("mjh_body_contact_force: n * nsel too large"); return MJH_ERR_ARG; }
  for (int s = 0; s < nsel; s++) {
    if (body[s] < 0 || body[s] >= e->M.nbody) { mjh_set_error("mjh_body_contact_force: body id out of range"); return MJH_ERR_ARG; }
    if (against && (against[s] < -1 || against[s] >= e->M.nbody)) { mjh_set_error("mjh_body_contact_force: `against` out of range"); return MJH_ERR_ARG; }
  }
  if ((size_t)e->R.maxcon * CF_STAGE * sizeof(float) > 64 * 1024) { mjh_set_error("mjh_body_contact_force: contact capacity beyond the kernel's LDS stage"); return MJH_ERR_CAPACITY; }
  return MJH_OK;
}
// the (checked) selection in e->csel_tab: uploaded in stream order from the engine's pinned buffer unless it is there already
static int body_force_table(mjh_engine* e, int nsel, const int* body, const int* against) {
  std::vector<int> want((size_t)2 * nsel);
  for (int s = 0; s < nsel; s++) { want[2*s] = body[s]; want[2*s+1] = against ? against[s] : -1; }
  if (e->csel_tab && want == e->csel_have) return MJH_OK;
  e->csel_have.clear();
  if (!e->csel_up) HIPCHK(hipEventCreateWithFlags(&e->csel_up, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(e->csel_up));      // (the last upload has read the host buffer)
  if (nsel > e->csel_cap) {
    if (e->csel_host) { HIPCHK(hipHostFree(e->csel_host)); e->csel_host = nullptr; }
    if (e->csel_tab) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(e->csel_tab)); e->csel_tab = nullptr; }
    e->csel_cap = 0;
    HIPCHK(hipHostMalloc((void**)&e->csel_host, (size_t)nsel * sizeof(int2), hipHostMallocDefault));
    HIPCHK(hipMalloc((void**)&e->csel_tab, (size_t)nsel * sizeof(int2)));
    e->csel_cap = nsel;
  }
  std::memcpy(e->csel_host, want.data(), want.size() * sizeof(int));
  HIPCHK(hipMemcpyAsync(e->csel_tab, e->csel_host, (size_t)nsel * sizeof(int2), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipEventRecord(e->csel_up, e->stream));
  e->csel_have = want;
  return MJH_OK;
}
extern "C" int mjh_body_contact_force_device(mjh_engine* e, int env0, int n, int nsel, const int* body, const int* against, void* d_force, void* d_count) {
  ENG(e); KEEP_HANDOVER(e);
  REPORT_ON(e, "mjh_body_contact_force_device");
  int rc = body_force_check(e, env0, n, nsel, body, against, d_force);
  if (rc) return rc;
  rc = body_force_table(e, nsel, body, against);
  if (rc) return rc;
  ContactForceArgs A{};
  A.ncon = e->R.ncon; A.rec = e->R.rec; A.geom_bodyid = e->dI + e->M.o_geom_bodyid; A.sel = e->csel_tab;
  A.force = (float*)d_force; A.count = (int*)d_count;
  A.env0 = env0; A.n = n; A.nsel = nsel; A.maxcon = e->R.maxcon; A.ngeom = e->M.ngeom;
  HIPCHK(mjh_launch_contact_force(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_body_contact_force(mjh_engine* e, int env0, int n, int nsel, const int* body, const int* against, double* force, int* count) {
  ENG(e); KEEP_HANDOVER(e);
  REPORT_ON(e, "mjh_body_contact_force");
  int rc = body_force_check(e, env0, n, nsel, body, against, force);
  if (rc) return rc;
  const size_t nout = (size_t)n * nsel;
  rc = io_reserve(e, &e->csel_io, &e->csel_io_words, 4 * nout);
  if (rc) return rc;
  float* const d_f = e->csel_io; int* const d_c = (int*)(e->csel_io + 3 * nout);
  rc = mjh_body_contact_force_device(e, env0, n, nsel, body, against, d_f, d_c);
  if (rc) return rc;
  std::vector<float> f(3 * nout);
  HIPCHK(hipMemcpyAsync(f.data(), d_f, f.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (count) HIPCHK(hipMemcpyAsync(count, d_c, nout * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < f.size(); i++) force[i] = f[i];
  return MJH_OK;
}
#undef REPORT_ON

// ---- frame states (mjh_frame_state / mjh_frame_state_device, frame.hip): the checks, the per-model tables at the first call, the frame table
// when it is not the last call's, the position-stage launch with the body poses (as fk_export issues it), then mjh_frame_state_kernel on the
// same stream.  Nothing of the envs' state, statistics or time is written.
// argument checks shared by both entry points: nothing is launched when one fails
// (accel: the rules of mjh_frame_accel — words = FRA_OUT per frame, MJH_FRAME_PROPER allowed, no ref, the LDS stage of FRA_STAGE words per dof)
static int frame_check(const mjh_engine* e, int env0, int n, int nframe, const mjh_frame* frames, const void* state, bool jac, bool accel = false) {
  const mjh_model* m = e->model;
  const char* const who = accel ? "mjh_frame_accel" : "mjh_frame_state";
  const auto fail = [who](const char* what, int rc) { mjh_set_error(std::string(who) + what); return rc; };
  if (env0 < 0 || n <= 0 || env0 + n > e->nenv) return fail(": env range out of bounds", MJH_ERR_ARG);
  if (nframe <= 0 || !frames || !state) return fail(": no frames or null pointer", MJH_ERR_ARG);
  if ((long long)n * nframe * (accel ? FRA_OUT : FR_STATE) > (1ll << 30)) return fail(": n * nframe too large", MJH_ERR_ARG);
  if (jac && (long long)n * nframe * 6 * (long long)m->nv > (1ll << 30)) return fail(": n * nframe * 6 * nv beyond 2^30", MJH_ERR_ARG);
  const int known = accel ? (MJH_FRAME_LOCAL | MJH_FRAME_PROPER) : MJH_FRAME_LOCAL;
  for (int f = 0; f < nframe; f++) {
    const mjh_frame& F = frames[f];
    if (F.objtype != MJH_FRAME_BODY && F.objtype != MJH_FRAME_SITE) return fail(": objtype is neither MJH_FRAME_BODY nor MJH_FRAME_SITE", MJH_ERR_ARG);
    if (F.id < 0 || F.id >= (F.objtype == MJH_FRAME_SITE ? m->nsite : m->nbody)) return fail(": frame id out of range", MJH_ERR_ARG);
    if (F.flags & ~known) return fail(": unknown flag", MJH_ERR_ARG);
    if (F.refid < -1) return fail(": bad ref", MJH_ERR_ARG);
    if (F.refid >= 0) {
      if (accel) return fail(": refid must be -1 (accelerations have no ref-relative form)", MJH_ERR_ARG);
      if (F.reftype != MJH_FRAME_BODY && F.reftype != MJH_FRAME_SITE) return fail(": reftype is neither MJH_FRAME_BODY nor MJH_FRAME_SITE", MJH_ERR_ARG);
      if (F.refid >= (F.reftype == MJH_FRAME_SITE ? m->nsite : m->nbody)) return fail(": ref id out of range", MJH_ERR_ARG);
      if (F.flags & MJH_FRAME_LOCAL) return fail(": MJH_FRAME_LOCAL together with a ref", MJH_ERR_ARG);
    }
  }
  if ((accel ? frame_acc_lds_bytes(m->nv) : frame_lds_bytes(m->nv)) > FR_LDS_MAX) return fail(": nv beyond the kernel's LDS stage", MJH_ERR_CAPACITY);
  return MJH_OK;
}
// the per-model tables of dev_frame.h, from the host model: one int buffer and one float buffer
static int frame_tables(mjh_engine* e) {
  if (e->frame_ready) return MJH_OK;
  const mjh_model* m = e->model;
  const int nv = m->nv, nb = m->nbody, nj = m->njnt, ns = m->nsite, nw = std::max(1, (nv + 31) / 32);
  const size_t o_dof = 0, o_body = o_dof + 4 * (size_t)nv, o_jnt = o_body + 4 * (size_t)nb, o_chain = o_jnt + 2 * (size_t)nj, o_site = o_chain + (size_t)nb * nw;
  std::vector<int> I(o_site + (size_t)ns + 4, 0);
  for (int d = 0; d < nv; d++) {
    const int j = m->dof_jntid[d];
    I[o_dof + 4*d] = m->jnt_type[j]; I[o_dof + 4*d + 1] = d - m->jnt_dofadr[j]; I[o_dof + 4*d + 2] = m->dof_bodyid[d]; I[o_dof + 4*d + 3] = j;
  }
  for (int b = 0; b < nb; b++) {
    I[o_body + 4*b] = m->body_parentid[b]; I[o_body + 4*b + 1] = m->body_jntadr[b]; I[o_body + 4*b + 2] = m->body_jntnum[b];
    I[o_body + 4*b + 3] = (m->nmocap > 0 && m->body_mocapid) ? m->body_mocapid[b] : -1;
    // the dofs that move the body: its own and its ancestors'
    for (int a = b; a > 0; a = m->body_parentid[a])
      for (int d = m->body_dofadr[a]; d < m->body_dofadr[a] + m->body_dofnum[a]; d++)
        if (d >= 0 && d < nv) I[o_chain + (size_t)b * nw + (d >> 5)] |= (int)(1u << (d & 31));
  }
  for (int j = 0; j < nj; j++) { I[o_jnt + 2*j] = m->jnt_type[j]; I[o_jnt + 2*j + 1] = m->jnt_qposadr[j]; }
  for (int s = 0; s < ns; s++) I[o_site + s] = m->site_bodyid[s];
  const size_t f_bpos = 0, f_bquat = f_bpos + 3 * (size_t)nb, f_jpos = f_bquat + 4 * (size_t)nb, f_jaxis = f_jpos + 3 * (size_t)nj, f_q0 = f_jaxis + 3 * (size_t)nj,
               f_spos = f_q0 + (size_t)m->nq, f_squat = f_spos + 3 * (size_t)ns;
  std::vector<float> F(f_squat + 4 * (size_t)ns + 4, 0.0f);
  for (int i = 0; i < 3 * nb; i++) F[f_bpos + i] = (float)m->body_pos[i];
  for (int i = 0; i < 4 * nb; i++) F[f_bquat + i] = (float)m->body_quat[i];
  for (int i = 0; i < 3 * nj; i++) { F[f_jpos + i] = (float)m->jnt_pos[i]; F[f_jaxis + i] = (float)m->jnt_axis[i]; }
  for (int i = 0; i < m->nq; i++) F[f_q0 + i] = (float)m->qpos0[i];
  for (int i = 0; i < 3 * ns; i++) F[f_spos + i] = (float)m->site_pos[i];
  for (int i = 0; i < 4 * ns; i++) F[f_squat + i] = (float)m->site_quat[i];
  int* dI = nullptr; float* dF = nullptr;
  int rc = dev_alloc(e, &dI, I.size(), false);
  if (!rc) rc = dev_alloc(e, &dF, F.size(), false);
  if (rc) return rc;
  HIPCHK(hipMemcpy(dI, I.data(), I.size() * sizeof(int), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dF, F.data(), F.size() * sizeof(float), hipMemcpyHostToDevice));
  FrameModel& M = e->frame_model;
  M.dof = (const int4*)(dI + o_dof); M.body = (const int4*)(dI + o_body); M.jnt = (const int2*)(dI + o_jnt);
  M.chain = (const unsigned*)(dI + o_chain); M.site_body = dI + o_site;
  M.body_pos = dF + f_bpos; M.body_quat = dF + f_bquat; M.jnt_pos = dF + f_jpos; M.jnt_axis = dF + f_jaxis; M.qpos0 = dF + f_q0;
  M.site_pos = dF + f_spos; M.site_quat = dF + f_squat;
  M.nv = nv; M.nbody = nb; M.njnt = nj; M.nsite = ns; M.nw = nw;
  e->frame_ready = true;
  return MJH_OK;
}
// the (checked) frames in T->tab (the state calls' table or the acceleration calls'): uploaded in stream order from the table's pinned
// buffer unless they are there already
static int frame_table(mjh_engine* e, mjh_engine::FrameTable* T, int nframe, const mjh_frame* frames) {
  std::vector<int> want((size_t)5 * nframe);
  for (int f = 0; f < nframe; f++) {
    const bool ref = frames[f].refid >= 0;
    want[5*f] = frames[f].objtype; want[5*f+1] = frames[f].id; want[5*f+2] = ref ? frames[f].reftype : 0; want[5*f+3] = ref ? frames[f].refid : -1; want[5*f+4] = frames[f].flags;
  }
  if (T->tab && want == T->have) return MJH_OK;
  T->have.clear();
  if (!T->up) HIPCHK(hipEventCreateWithFlags(&T->up, hipEventDisableTiming));
  else HIPCHK(hipEventSynchronize(T->up));      // (the last upload has read the host buffer)
  if (nframe > T->cap) {
    if (T->host) { HIPCHK(hipHostFree(T->host)); T->host = nullptr; }
    if (T->tab) { HIPCHK(hipStreamSynchronize(e->stream)); HIPCHK(hipFree(T->tab)); T->tab = nullptr; }
    T->cap = 0;
    HIPCHK(hipHostMalloc((void**)&T->host, (size_t)nframe * sizeof(FrameRec), hipHostMallocDefault));
    HIPCHK(hipMalloc((void**)&T->tab, (size_t)nframe * sizeof(FrameRec)));
    T->cap = nframe;
  }
  const mjh_model* m = e->model;
  for (int f = 0; f < nframe; f++) {
    const mjh_frame& F = frames[f];
    FrameRec R{};
    R.site = F.objtype == MJH_FRAME_SITE ? F.id : -1; R.body = R.site >= 0 ? m->site_bodyid[R.site] : F.id;
    R.ref = F.refid >= 0 ? 1 : 0; R.rbody = 0; R.rsite = -1;
    if (R.ref) { R.rsite = F.reftype == MJH_FRAME_SITE ? F.refid : -1; R.rbody = R.rsite >= 0 ? m->site_bodyid[R.rsite] : F.refid; }
    R.local = (F.flags & MJH_FRAME_LOCAL) ? 1 : 0;
    R.proper = (F.flags & MJH_FRAME_PROPER) ? 1 : 0;
    T->host[f] = R;
  }
  HIPCHK(hipMemcpyAsync(T->tab, T->host, (size_t)nframe * sizeof(FrameRec), hipMemcpyHostToDevice, e->stream));
  HIPCHK(hipEventRecord(T->up, e->stream));
  T->have = want;
  return MJH_OK;
}
// the position-stage launch of the env range with the body poses, as fk_export issues it: xpos [n][nbody][3] at the engine's export scratch,
// xquat [n][nbody][4] *fx floats behind it
static int frame_poses(mjh_engine* e, int env0, int n, size_t* fx) {
  const int nb = e->M.nbody;
  *fx = (size_t)n * 3 * nb;
  int rc = ensure_scratch(e, *fx + (size_t)n * 4 * nb);
  if (rc) return rc;
  StateGuard guard(&e->S);
  e->S.x_xpos = e->scratch; e->S.x_xquat = e->scratch + *fx;
  return launch(e, env0, n, 1, PH_FKONLY, XF_BODY);
}
extern "C" int mjh_frame_state_device(mjh_engine* e, int env0, int n, int nframe, const mjh_frame* frames, void* d_state, void* d_jac) {
  ENG(e);
  int rc = frame_check(e, env0, n, nframe, frames, d_state, d_jac != nullptr);
  if (rc) return rc;
  rc = frame_tables(e);
  if (!rc) rc = frame_table(e, &e->frame_tab, nframe, frames);
  size_t fx = 0;
  if (!rc) rc = frame_poses(e, env0, n, &fx);
  if (rc) return rc;
  FrameArgs A{};
  A.M = e->frame_model;
  A.xpos = e->scratch; A.xquat = e->scratch + fx; A.qpos = e->S.qpos; A.qvel = e->S.qvel; A.frames = e->frame_tab.tab;
  A.state = (float*)d_state; A.jac = (float*)d_jac;
  A.env0 = env0; A.n = n; A.nframe = nframe; A.nqp = e->M.nqp; A.nvp = e->M.nvp;
  HIPCHK(mjh_launch_frame_state(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_frame_state(mjh_engine* e, int env0, int n, int nframe, const mjh_frame* frames, double* state, double* jac) {
  ENG(e);
  int rc = frame_check(e, env0, n, nframe, frames, state, jac != nullptr);
  if (rc) return rc;
  const size_t ns = (size_t)n * nframe * FR_STATE, nj = jac ? (size_t)n * nframe * 6 * (size_t)e->M.nv : 0;
  rc = io_reserve(e, &e->frame_io, &e->frame_io_floats, ns + nj);
  if (rc) return rc;
  float* const d_s = e->frame_io; float* const d_j = nj ? e->frame_io + ns : nullptr;
  rc = mjh_frame_state_device(e, env0, n, nframe, frames, d_s, jac ? (void*)(nj ? d_j : d_s) : nullptr);
  if (rc) return rc;
  std::vector<float> h(ns + nj);
  HIPCHK(hipMemcpyAsync(h.data(), d_s, h.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < ns; i++) state[i] = h[i];
  for (size_t i = 0; i < nj; i++) jac[i] = h[ns + i];
  return MJH_OK;
}

// ---- frame accelerations (mjh_frame_accel / mjh_frame_accel_device, frame_acc.hip): the checks, the per-model tables and the launch pattern
// of the frame states (a frame table of their own), then mjh_frame_accel_kernel on the same stream with the engine's qacc of the last solve.
// Nothing of the envs' state, statistics or time is written.
extern "C" int mjh_frame_accel_device(mjh_engine* e, int env0, int n, int nframe, const mjh_frame* frames, void* d_acc, void* d_bias) {
  ENG(e);
  int rc = frame_check(e, env0, n, nframe, frames, d_acc, false, true);
  if (rc) return rc;
  rc = frame_tables(e);
  if (!rc) rc = frame_table(e, &e->facc_tab, nframe, frames);
  size_t fx = 0;
  if (!rc) rc = frame_poses(e, env0, n, &fx);
  if (rc) return rc;
  FrameAccArgs A{};
  A.M = e->frame_model;
  A.xpos = e->scratch; A.xquat = e->scratch + fx; A.qpos = e->S.qpos; A.qvel = e->S.qvel; A.qacc = e->S.qacc; A.frames = e->facc_tab.tab;
  A.acc = (float*)d_acc; A.bias = (float*)d_bias;
  const bool grav = !(e->M.disableflags & MJH_DSBL_GRAVITY);      // (the gravity the step kernels take)
  for (int k = 0; k < 3; k++) A.gravity[k] = grav ? e->M.gravity[k] : 0.0f;
  A.env0 = env0; A.n = n; A.nframe = nframe; A.nqp = e->M.nqp; A.nvp = e->M.nvp;
  HIPCHK(mjh_launch_frame_accel(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_frame_accel(mjh_engine* e, int env0, int n, int nframe, const mjh_frame* frames, double* acc, double* bias) {
  ENG(e);
  int rc = frame_check(e, env0, n, nframe, frames, acc, false, true);
  if (rc) return rc;
  const size_t na = (size_t)n * nframe * FRA_OUT, nb = bias ? na : 0;
  rc = io_reserve(e, &e->facc_io, &e->facc_io_floats, na + nb);
  if (rc) return rc;
  rc = mjh_frame_accel_device(e, env0, n, nframe, frames, e->facc_io, bias ? e->facc_io + na : nullptr);
  if (rc) return rc;
  std::vector<float> h(na + nb);
  HIPCHK(hipMemcpyAsync(h.data(), e->facc_io, h.size() * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  for (size_t i = 0; i < na; i++) acc[i] = h[i];
  for (size_t i = 0; i < nb; i++) bias[i] = h[na + i];
  return MJH_OK;
}

// ---- height scans (mjh_heightscan / mjh_heightscan_device, heightscan.hip): the checks (dev_heightscan.h), the root-id table at the first
// call with exclude_tree = 1, ray_scene() (with the body poses when the sensor is a site), then mjh_heightscan_kernel on the same stream.
extern "C" void mjh_heightscan_default_options(mjh_heightscan_options* o) {
  if (!o) return;
  o->site = -1; o->align = MJH_HSCAN_ALIGN_YAW; o->width = 16; o->height = 16;
  o->spacing[0] = 0.1; o->spacing[1] = 0.1; o->offset[0] = 0.0; o->offset[1] = 0.0; o->above = 1.0;
  o->bodyexclude = -1; o->exclude_tree = 0; o->flg_static = 1; o->cull = 1; o->cutoff = 0.0;
}
// argument checks shared by both entry points: nothing is launched when one fails
static int hscan_check(const mjh_engine* e, int env0, int n, const mjh_heightscan_options& o, const void* range) {
  if (const char* bad = hscan_args_error(e->model->nsite, e->model->nbody, e->nenv, env0, n, o, range)) {
    mjh_set_error(std::string("mjh_heightscan: ") + bad); return MJH_ERR_ARG;
  }
  return MJH_OK;
}
extern "C" int mjh_heightscan_device(mjh_engine* e, int env0, int n, const mjh_heightscan_options* opt, float* d_range, int* d_geomid, float* d_points) {
  ENG(e);
  mjh_heightscan_options o; mjh_heightscan_default_options(&o);
  if (opt) o = *opt;
  int rc = hscan_check(e, env0, n, o, d_range);
  if (rc) return rc;
  const mjh_model* m = e->model;
  if (o.exclude_tree && !e->hscan_root) {
    int* root = nullptr;
    HIPCHK(hipMalloc((void**)&root, (size_t)m->nbody * sizeof(int)));
    const hipError_t filled = hipMemcpy(root, m->body_rootid, (size_t)m->nbody * sizeof(int), hipMemcpyHostToDevice);
    if (filled != hipSuccess) (void)hipFree(root);
    HIPCHK(filled);
    e->hscan_root = root;      // (only a table that was filled is kept)
  }
  HScanArgs A{};
  rc = ray_scene(e, env0, n, o.site >= 0, o.bodyexclude, o.flg_static, o.cutoff, &A.W, &A.T);
  if (rc) return rc;
  A.range = d_range; A.geomid = d_geomid; A.points = d_points;
  A.width = o.width; A.height = o.height; A.tw_log = scan_tile_shape(o.height); A.cull = o.cull ? 1 : 0; A.align = o.align;
  A.ox = (float)o.offset[0]; A.oy = (float)o.offset[1]; A.hx = (float)(0.5 * o.spacing[0]); A.hy = (float)(0.5 * o.spacing[1]);
  A.above = (float)o.above;
  A.rootid = o.exclude_tree ? e->hscan_root : nullptr; A.root_ex = o.exclude_tree ? m->body_rootid[o.bodyexclude] : -1;
  site_frame(m, o.site, &A);
  HIPCHK(mjh_launch_heightscan(e->stream, A));
  return MJH_OK;
}
extern "C" int mjh_heightscan(mjh_engine* e, int env0, int n, const mjh_heightscan_options* opt, float* range, int* geomid, float* points) {
  ENG(e);
  mjh_heightscan_options o; mjh_heightscan_default_options(&o);
  if (opt) o = *opt;
  int rc = hscan_check(e, env0, n, o, range);
  if (rc) return rc;
  return scan_readback(e, (size_t)n * o.width * o.height, range, geomid, points,
                       [&](float* d_range, int* d_geomid, float* d_points) { return mjh_heightscan_device(e, env0, n, &o, d_range, d_geomid, d_points); });
}

// ---- RGB-D images (mjh_render / mjh_render_device, render.hip): the depth launch exactly as mjh_depth_device issues it — into the
// caller's buffers, or into engine-owned scratch where the caller takes neither image — then mjh_shade_kernel on the same stream.
extern "C" void mjh_render_default_options(mjh_render_options* o) {
  if (!o) return;
  mjh_depth_default_options(&o->view);
  o->ambient = 0.3f; o->diffuse = 0.7f;
  for (int k = 0; k < 4; k++) o->background[k] = 0.0f;
}
// argument checks shared by both entry points: nothing is launched when one fails
static int render_check(const mjh_engine* e, int env0, int n, const mjh_render_options& o, const void* depth, const void* geomid, const void* normal, const void* rgba) {
  if (!depth && !geomid && !normal && !rgba) { mjh_set_error("mjh_render: every output pointer is null"); return MJH_ERR_ARG; }
  if (!(o.ambient >= 0.0f && std::isfinite(o.ambient) && o.diffuse >= 0.0f && std::isfinite(o.diffuse))) { mjh_set_error("mjh_render: ambient and diffuse must be finite and not negative"); return MJH_ERR_ARG; }
  for (int k = 0; k < 4; k++) if (!(o.background[k] >= 0.0f && o.background[k] <= 1.0f)) { mjh_set_error("mjh_render: background components must lie in [0, 1]"); return MJH_ERR_ARG; }
  return depth_check(e, env0, n, o.view, depth, !(normal || rgba));      // (with a normal or colour image the depth image is optional)
}
static int render_tables(mjh_engine* e) {
  if (e->ray_color) return MJH_OK;
  const mjh_model* m = e->model;
  std::vector<float4> col((size_t)std::max(m->ngeom, 1), make_float4(0.5f, 0.5f, 0.5f, 1.0f));      // (a model assembled from tables has no geom_rgba: the default)
  if (m->geom_rgba) for (int g = 0; g < m->ngeom; g++) col[g] = make_float4((float)m->geom_rgba[4*g], (float)m->geom_rgba[4*g+1], (float)m->geom_rgba[4*g+2], (float)m->geom_rgba[4*g+3]);
  float4* d = nullptr;
  int rc = dev_alloc(e, &d, col.size(), false);
  if (rc) return rc;
  HIPCHK(hipMemcpy(d, col.data(), col.size() * sizeof(float4), hipMemcpyHostToDevice));
  e->ray_color = d;
  return MJH_OK;
}
// ---- lights (include/mjhip.h: mjh_render_set_lighting).  The model's lights as kernel records, once per engine.
static void light_tables(mjh_engine* e) {
  if (e->lights_ready) return;
  const mjh_model* m = e->model;
  e->nlight = std::min(std::max(m->nlight, 0), MJH_MAXLIGHT);
  for (int l = 0; l < e->nlight; l++) {
    LightRec& R = e->lights[l];
    R.body = m->light_bodyid[l];
    R.flags = (m->light_directional[l] ? LIGHT_DIRECTIONAL : 0) | (m->light_castshadow[l] ? LIGHT_CASTSHADOW : 0);
    for (int k = 0; k < 3; k++) {
      R.pos[k] = (float)m->light_pos[3*l + k]; R.dir[k] = (float)m->light_dir[3*l + k];
      R.dif[k] = (float)m->light_diffuse[3*l + k]; R.amb[k] = (float)m->light_ambient[3*l + k];
    }
    R.coscut = (float)std::cos(m->light_cutoff[l] * 3.14159265358979323846 / 180.0); R.exponent = (float)m->light_exponent[l];
    e->light_on[l] = m->light_active[l] ? 1 : 0;
  }
  e->lights_ready = true;
}
extern "C" void mjh_light_default_options(mjh_light_options* o) { if (o) { o->shadows = 1; o->cull = 1; o->bias = 1e-3f; } }
extern "C" int mjh_render_set_lighting(mjh_engine* e, int mode) {
  ENG_NOJOIN(e);
  if (mode != 0 && mode != 1) { mjh_set_error("mjh_render_set_lighting: mode must be 0 or 1"); return MJH_ERR_ARG; }
  e->light_mode = mode;
  return MJH_OK;
}
extern "C" int mjh_render_get_lighting(const mjh_engine* e) { return e ? e->light_mode : 0; }
extern "C" int mjh_render_set_light_options(mjh_engine* e, const mjh_light_options* o) {
  ENG_NOJOIN(e);
  if (!o) { mjh_set_error("mjh_render_set_light_options: null pointer"); return MJH_ERR_ARG; }
  if ((o->shadows != 0 && o->shadows != 1) || (o->cull != 0 && o->cull != 1)) { mjh_set_error("mjh_render_set_light_options: shadows and cull must be 0 or 1"); return MJH_ERR_ARG; }
  if (!(o->bias > 0.0f && std::isfinite(o->bias))) { mjh_set_error("mjh_render_set_light_options: bias must be positive and finite"); return MJH_ERR_ARG; }
  e->light_opt = *o;
  return MJH_OK;
}
extern "C" int mjh_render_get_light_options(const mjh_engine* e, mjh_light_options* o) {
  if (!e || !o) { mjh_set_error("mjh_render_get_light_options: null pointer"); return MJH_ERR_ARG; }
  *o = e->light_opt;
  return MJH_OK;
}
extern "C" int mjh_set_light_active(mjh_engine* e, int light, int on) {
  ENG_NOJOIN(e);
  light_tables(e);
  if (light < 0 || light >= e->nlight) { mjh_set_error("mjh_set_light_active: light id out of range"); return MJH_ERR_ARG; }
  e->light_on[light] = on ? 1 : 0;
  return MJH_OK;
}

// ---- textures (include/mjhip.h: mjh_render_set_texturing).  The geoms' texture records and the texel table, once per engine.
static int texture_tables(mjh_engine* e) {
  if (e->tex_rec) return MJH_OK;
  const mjh_model* m = e->model;
  std::vector<TexRec> rec((size_t)std::max(m->ngeom, 1), TexRec{-1, 0, 1, 1, 1.0f, 1.0f, 0, 0});
  for (int g = 0; g < m->ngeom; g++) {
    const int t = m->geom_texid ? m->geom_texid[g] : -1;
    if (t < 0 || t >= m->ntex) continue;
    const long long adr = m->tex_adr[t], w = m->tex_width[t], h = m->tex_height[t];
    if (w < 1 || h < 1 || adr < 0 || adr + w * h > (long long)m->ntexdata) { mjh_set_error("mjh_render: texture table out of range"); return MJH_ERR_ARG; }
    rec[g] = TexRec{t, (int)adr, (int)w, (int)h, (float)m->geom_texrepeat[2*g], (float)m->geom_texrepeat[2*g+1], m->geom_texuniform[g] ? 1 : 0, 0};
  }
  std::vector<unsigned> tex((size_t)m->ntexdata);
  for (size_t i = 0; i < tex.size(); i++) tex[i] = (unsigned)m->tex_rgb[3*i] | ((unsigned)m->tex_rgb[3*i+1] << 8) | ((unsigned)m->tex_rgb[3*i+2] << 16) | TEXEL_FLAG;
  TexRec* dr = nullptr; unsigned* dt = nullptr;
  int rc = dev_alloc(e, &dt, tex.size(), false);
  if (rc) return rc;
  rc = dev_alloc(e, &dr, rec.size(), false);
  if (rc) return rc;
  HIPCHK(hipMemcpy(dt, tex.data(), tex.size() * sizeof(unsigned), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dr, rec.data(), rec.size() * sizeof(TexRec), hipMemcpyHostToDevice));
  e->tex_data = dt; e->tex_rec = dr;
  return MJH_OK;
}
extern "C" int mjh_render_set_texturing(mjh_engine* e, int mode) {
  ENG_NOJOIN(e);
  if (mode != 0 && mode != 1) { mjh_set_error("mjh_render_set_texturing: mode must be 0 or 1"); return MJH_ERR_ARG; }
  e->tex_mode = mode;
  return MJH_OK;
}
extern "C" int mjh_render_get_texturing(const mjh_engine* e) { return e ? e->tex_mode : 0; }

extern "C" int mjh_render_device(mjh_engine* e, int env0, int n, const mjh_render_options* opt, float* d_depth, int* d_geomid, float* d_normal, unsigned char* d_rgba) {
  ENG(e);
  mjh_render_options o; mjh_render_default_options(&o);
  if (opt) o = *opt;
  int rc = render_check(e, env0, n, o, d_depth, d_geomid, d_normal, d_rgba);
  if (rc) return rc;
  if (!d_normal && !d_rgba) return mjh_depth_device(e, env0, n, &o.view, d_depth, d_geomid);
  rc = render_tables(e);
  if (rc) return rc;
  // lighting mode 1 with a colour image and an active light: the shade launch writes the normal only, the light kernel the colour
  LightArgs LA{};
  if (e->light_mode == 1 && d_rgba) {
    light_tables(e);
    for (int l = 0; l < e->nlight; l++) if (e->light_on[l]) LA.L[LA.nlight++] = e->lights[l];
  }
  const bool lit = LA.nlight > 0;
  const size_t nout = (size_t)n * o.view.width * o.view.height;
  if (!d_depth || !d_geomid || (lit && !d_normal)) {
    rc = io_reserve(e, &e->render_io, &e->render_io_floats, (lit && !d_normal ? 5 : 2) * nout);
    if (rc) return rc;
    if (!d_depth) d_depth = e->render_io;
    if (!d_geomid) d_geomid = (int*)(e->render_io + nout);
    if (lit && !d_normal) d_normal = e->render_io + 2 * nout;
  }
  // texturing mode 1 with a colour image and a textured model: the texture kernel writes the texel image between the depth and shade launches
  const bool textured = e->tex_mode == 1 && d_rgba && e->model->ntex > 0 && e->model->ntexdata > 0;
  unsigned* d_texel = nullptr;
  if (textured) {
    rc = texture_tables(e);
    if (rc) return rc;
    rc = io_reserve(e, &e->tex_io, &e->tex_io_floats, nout);
    if (rc) return rc;
    d_texel = (unsigned*)e->tex_io;
  }
  ShadeArgs A{};
  rc = depth_chain(e, env0, n, o.view, d_depth, d_geomid, &A.D);
  if (rc) return rc;
  HIPCHK(mjh_launch_depth(e->stream, A.D));
  if (textured) {
    TextureArgs TA{};
    TA.D = A.D; TA.rec = e->tex_rec; TA.texels = e->tex_data; TA.ntexdata = e->model->ntexdata; TA.out = d_texel;
    HIPCHK(mjh_launch_texture(e->stream, TA));
  }
  A.texel = lit ? nullptr : d_texel;
  A.color = e->ray_color; A.normal = d_normal; A.rgba = lit ? nullptr : (unsigned*)d_rgba;
  A.ambient = o.ambient; A.diffuse = o.diffuse;
  A.background = render_pack(o.background[0], o.background[1], o.background[2], o.background[3]);
  HIPCHK(mjh_launch_shade(e->stream, A));
  if (lit) {
    LA.texel = d_texel;
    LA.D = A.D; LA.color = e->ray_color; LA.normal = d_normal; LA.rgba = (unsigned*)d_rgba;
    LA.ambient = o.ambient; LA.diffuse = o.diffuse; LA.background = A.background;
    LA.shadows = e->light_opt.shadows; LA.cull = e->light_opt.cull; LA.bias = e->light_opt.bias;
    HIPCHK(mjh_launch_light(e->stream, LA));
  }
  return MJH_OK;
}
extern "C" int mjh_render(mjh_engine* e, int env0, int n, const mjh_render_options* opt, float* depth, int* geomid, float* normal, unsigned char* rgba) {
  ENG(e);
  mjh_render_options o; mjh_render_default_options(&o);
  if (opt) o = *opt;
  int rc = render_check(e, env0, n, o, depth, geomid, normal, rgba);
  if (rc) return rc;
  if (!normal && !rgba) return mjh_depth(e, env0, n, &o.view, depth, geomid);
  const size_t nout = (size_t)n * o.view.width * o.view.height;
  rc = ray_io_reserve(e, 6 * nout);
  if (rc) return rc;
  float* const d_depth = e->ray_io; int* const d_gid = (int*)(e->ray_io + nout); float* const d_normal = e->ray_io + 2 * nout;
  unsigned char* const d_rgba = (unsigned char*)(e->ray_io + 5 * nout);
  // (lighting mode 1: the light kernel reads the normal image; the staging buffer has room for it whether or not the caller takes it)
  rc = mjh_render_device(e, env0, n, &o, d_depth, d_gid, (normal || (rgba && e->light_mode == 1)) ? d_normal : nullptr, rgba ? d_rgba : nullptr);
  if (rc) return rc;
  if (depth) HIPCHK(hipMemcpyAsync(depth, d_depth, nout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (geomid) HIPCHK(hipMemcpyAsync(geomid, d_gid, nout * sizeof(int), hipMemcpyDeviceToHost, e->stream));
  if (normal) HIPCHK(hipMemcpyAsync(normal, d_normal, 3 * nout * sizeof(float), hipMemcpyDeviceToHost, e->stream));
  if (rgba) HIPCHK(hipMemcpyAsync(rgba, d_rgba, nout * sizeof(unsigned), hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return MJH_OK;
}

extern "C" int mjh_nenv(const mjh_engine* e) { return e ? e->nenv : 0; }
extern "C" const mjh_model* mjh_engine_model(const mjh_engine* e) { return e ? e->model : nullptr; }
extern "C" int mjh_lds_bytes(const mjh_engine* e) { return e ? e->lds_bytes : 0; }
extern "C" int mjh_solver_order(const mjh_engine* e) { return !e ? 0 : e->M.pgs_row_order ? 2 : e->M.patch ? 1 : 0; }
extern "C" int mjh_pgs_schedule(const mjh_engine* e) { return !e ? 0 : e->M.pgs_row_order; }
extern "C" int mjh_patch_sweep(const mjh_engine* e) { return !e ? 0 : e->M.patch; }
extern "C" int mjh_window_solver(const mjh_engine* e) { return !e ? 0 : (e->M.window && e->S.wbuf ? 1 : 0); }
extern "C" int mjh_dense_solver(const mjh_engine* e) { return e && e->M.big && e->split3 && e->M.dense ? 1 : 0; }
extern "C" const char* mjh_version(void) { return "mjhip 0.1 (gfx950)"; }
