// control.hip — commands, joint state and resets between a caller's device buffers and the engine's per-env rows (mjh_set_cmd_device,
// mjh_set_pd_target_device, mjh_set_xfrc_applied_device, mjh_get_joint_state_device, mjh_reset_device, mjh_reset with an id list).
// The host side (checks, stream choice, first-use allocations) is in engine.hip; nothing here waits for the device.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/mjhip.h"
#include "dev_control.h"

// Row moves: one thread per float of the dense side, grid-stride; consecutive lanes touch consecutive floats of the dense buffer and of the
// engine's row (a row boundary breaks the run once per `width` floats).  Bits are copied, nothing is converted.  Indices are size_t: n * width
// of the widest table (6 nbody of a large model over thousands of envs) stays far below 2^31, the byte offsets behind it need not.
template <bool SCATTER>
__global__ __launch_bounds__(256) void mjh_control_rows_kernel(const ControlRowsArgs A) {
  const size_t n = (size_t)A.n;
  const size_t t0 = n * (size_t)A.width[0], t1 = t0 + n * (size_t)A.width[1], t2 = t1 + n * (size_t)A.width[2];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < t2; i += (size_t)gridDim.x * blockDim.x) {
    const int k = i < t0 ? 0 : (i < t1 ? 1 : 2);
    const size_t j = i - (k == 0 ? 0 : (k == 1 ? t0 : t1));
    const size_t w = (size_t)A.width[k], row = j / w, col = j - row * w;
    float* const pe = A.eng[k] + ((size_t)A.env0 + row) * (size_t)A.stride[k] + col;
    float* const pb = A.buf[k] + j;
    if (SCATTER) *pe = *pb; else *pb = *pe;
  }
}

static hipError_t launch_rows(hipStream_t st, const ControlRowsArgs& A, bool scatter) {
  if (A.n <= 0 || A.env0 < 0) return hipErrorInvalidValue;
  size_t total = 0;
  for (int k = 0; k < CTL_MAXPART; k++) {
    if (A.width[k] < 0 || (A.width[k] > 0 && (!A.eng[k] || !A.buf[k] || A.stride[k] < A.width[k]))) return hipErrorInvalidValue;
    total += (size_t)A.n * (size_t)A.width[k];
  }
  if (total == 0) return hipSuccess;
  const unsigned blocks = (unsigned)std::min<size_t>((total + 255) / 256, 4096);
  if (scatter) hipLaunchKernelGGL(mjh_control_rows_kernel<true>, dim3(blocks), dim3(256), 0, st, A);
  else hipLaunchKernelGGL(mjh_control_rows_kernel<false>, dim3(blocks), dim3(256), 0, st, A);
  return hipGetLastError();
}
hipError_t mjh_launch_scatter_rows(hipStream_t st, const ControlRowsArgs& A) { return launch_rows(st, A, true); }
hipError_t mjh_launch_gather_rows(hipStream_t st, const ControlRowsArgs& A) { return launch_rows(st, A, false); }

// Reset: one wavefront per row of the launch (an env of the range, or an entry of the id list), four per block.  The mask byte / the id is
// made wave-uniform before the branch, so an env that is not selected costs its wavefront one byte load and an exit.  A selected env gets
// what PH_RESET of the step kernel writes (step_kernel.h), field by field: the lanes stride over the env's rows, which start on 128-byte
// lines (qvel / qacc_warmstart / ddq / dq are columns of the qpos record: one run of lines), so the stores are whole lines.  Plain vector
// stores, no LDS, no atomics.
__global__ __launch_bounds__(256) void mjh_reset_rows_kernel(const ControlResetArgs A) {
  const DModel& M = A.C->M;
  const DState& S = A.S;
  const int lane = (int)(threadIdx.x & 63);
  const size_t row = (size_t)blockIdx.x * 4 + (size_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (row >= (size_t)A.n) return;
  int env;
  if (A.ids) env = __builtin_amdgcn_readfirstlane(A.ids[row]);
  else {
    if (A.mask && __builtin_amdgcn_readfirstlane((int)A.mask[row]) == 0) return;
    env = A.env0 + (int)row;
  }
  const int nq = M.nq, nv = M.nv, nbody = M.nbody;
  const size_t qrow = (size_t)env * (size_t)M.nqp, vrow = (size_t)env * (size_t)M.nvp;
  const float* const q_in = A.qpos ? A.qpos + row * (size_t)nq : S.initial_qpos + qrow;
  const float* const v_in = A.qvel ? A.qvel + row * (size_t)nv : nullptr;
  for (int i = lane; i < nq; i += 64) S.qpos[qrow + i] = q_in[i];
  for (int i = lane; i < nv; i += 64) {
    S.qvel[vrow + i] = v_in ? v_in[i] : 0.0f; S.qacc_ws[vrow + i] = 0; S.qvel_ref[vrow + i] = 0; S.qfrc_applied[vrow + i] = 0;
    S.ddq[vrow + i] = 0; S.dq[vrow + i] = 0;
  }
  if (lane == 0) { S.time[env] = 0; S.stats[4 * (size_t)env] = 0; S.stats[4 * (size_t)env + 1] = 0; S.stats[4 * (size_t)env + 2] = 0; S.stats[4 * (size_t)env + 3] = 0; }
  // the env's contact report: as before the first solve.  (Written by the articulated instances of the step kernel only, and cleared by the
  // same ones under PH_RESET: a model with a diagonal mass matrix keeps what it has, there as here.)
  const DReport& R = A.C->R;
  if (R.on && !M.diagM) {
    const size_t words = (size_t)R.maxcon * CREP_STRIDE;
    float* const rec = R.rec + (size_t)env * words;
    for (size_t i = lane; i < words; i += 64) rec[i] = 0;
    float* const cf = R.cfrc + (size_t)env * (size_t)(6 * nbody);
    for (int i = lane; i < 6 * nbody; i += 64) cf[i] = 0;
    if (lane == 0) R.ncon[env] = 0;
  }
}

hipError_t mjh_launch_reset_rows(hipStream_t st, const ControlResetArgs& A) {
  if (A.n <= 0 || A.env0 < 0 || !A.C || (A.ids && (A.mask || A.qpos || A.qvel))) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mjh_reset_rows_kernel, dim3((unsigned)(((size_t)A.n + 3) / 4)), dim3(256), 0, st, A);
  return hipGetLastError();
}
