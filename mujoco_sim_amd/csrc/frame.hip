// frame.hip — mjh_frame_state_kernel: world pose, twist and Jacobian of selected bodies and sites of every env, from the body poses the
// position-stage launch exported (PH_FKONLY with XF_BODY) and the envs' qpos / qvel.  A translation unit of its own: no instance of the
// step kernels is touched.  Stream-ordered behind the steps queued so far; nothing of the envs' state is written.  gfx950 only.
#include <hip/hip_runtime.h>

// No contraction anywhere in this unit, the helpers of dev_math.h included: every product and sum is rounded as written, so that a frame's
// numbers are a function of the env's state and the frame alone — whichever call, position in the frame table or output selection the
// compiler specialises a copy of the walk for.
#pragma clang fp contract(off)

#include "../../include/mjhip.h"
#include "dev_frame.h"
#include "dev_math.h"

#define U(x) __builtin_amdgcn_readfirstlane(x)      // a wave-uniform integer, kept in a scalar register

// (frame_pose and the stage loop of the kernel below have a twin in frame_acc.hip — facc_pose, facc_column — written operation for operation
// the same, so that both units form the same column bits: an edit here is made there too; tests/test_gpu_frame_acc.py compares the bits)
// world pose of (body, site): the exported body pose; a site adds its offset as the step kernel's site frames do
static __device__ __forceinline__ void frame_pose(const FrameArgs& A, const float* xp, const float* xq, int body, int site, float p[3], float q[4]) {
  const float* bp = xp + 3 * body; const float* bq = xq + 4 * body;
  if (site < 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = bp[k];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = bq[k];
  } else {
    float m[9], t[3];
    quat2mat(m, bq); rotvec(t, m, A.M.site_pos + 3 * site);
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = bp[k] + t[k];
    mulquat(q, bq, A.M.site_quat + 4 * site);
  }
}

// Twist of the point p of `body` in world axes, and optionally the Jacobian rows (jac: [6][nv] of this env and frame).  Lanes = dofs:
// a lane whose dof is in the body's chain forms its column from the LDS stage and p, the others hold zeros; every lane adds
// column * qvel over d = lane, lane + 64, .. in ascending order, then one butterfly over the wavefront.
static __device__ __forceinline__ void frame_twist(const FrameArgs& A, const float* s, int lane, int body, const float p[3], float* jac,
                                                   float v[3], float w[3]) {
  const int nv = A.M.nv, nw = A.M.nw;
  const unsigned* mk = A.M.chain + (size_t)body * nw;
  float acc[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  for (int d0 = 0; d0 < nv; d0 += 64) {
    const int d = d0 + lane, wi = d0 >> 5;
    const unsigned lo = U(mk[wi]), hi = wi + 1 < nw ? U(mk[wi + 1]) : 0u;
    const bool in = d < nv && (((lane < 32 ? lo : hi) >> (lane & 31)) & 1u);
    float c[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float qv = 0.0f;
    if (in) {
      const float ax[3] = {s[d], s[nv + d], s[2 * nv + d]};
      if (__float_as_int(s[6 * nv + d])) {
        const float r[3] = {p[0] - s[3 * nv + d], p[1] - s[4 * nv + d], p[2] - s[5 * nv + d]};
        cross3(c, ax, r);
        c[3] = ax[0]; c[4] = ax[1]; c[5] = ax[2];
      } else { c[0] = ax[0]; c[1] = ax[1]; c[2] = ax[2]; }
      qv = s[7 * nv + d];
    }
    if (jac && d < nv) {
#pragma unroll
      for (int r = 0; r < 6; r++) jac[(size_t)r * nv + d] = c[r];
    }
#pragma unroll
    for (int r = 0; r < 6; r++) acc[r] += c[r] * qv;
  }
#pragma unroll
  for (int r = 0; r < 6; r++) acc[r] = frame_wave_sum(acc[r]);
  v[0] = acc[0]; v[1] = acc[1]; v[2] = acc[2]; w[0] = acc[3]; w[1] = acc[4]; w[2] = acc[5];
}

// One workgroup (one wavefront) per env.  Stage: lanes = dofs form their dof's kind, world axis and world anchor, once per env, from the
// PARENT's exported pose, body_pos / body_quat and the body's own joints up to their own, in mj_kinematics' order (a free joint's from the
// body's own pose), and keep them in LDS beside qvel (FR_STAGE words per dof, one array per word: conflict-free over d).  Walk: the loop over
// the frames is wave-uniform (frame_twist).  A ref frame's pose and twist come from the same walk, then the relative forms are applied.
__global__ __launch_bounds__(64) void mjh_frame_state_kernel(const FrameArgs A) {
  extern __shared__ float s_stage[];
  const int lane = (int)threadIdx.x, row = (int)blockIdx.x;
  if (row >= A.n) return;
  const int env = A.env0 + row, nv = A.M.nv, nb = A.M.nbody;
  const float* const xp = A.xpos + (size_t)row * 3 * nb;
  const float* const xq = A.xquat + (size_t)row * 4 * nb;
  const float* const qpos = A.qpos + (size_t)env * A.nqp;
  const float* const qvel = A.qvel + (size_t)env * A.nvp;
  for (int d = lane; d < nv; d += 64) {
    const int4 D = A.M.dof[d];
    const int b = D.z;
    float axis[3] = {0.0f, 0.0f, 0.0f}, anchor[3] = {0.0f, 0.0f, 0.0f};
    int kind = 0;
    if (D.x == MJH_JNT_FREE) {
      if (D.y < 3) { axis[0] = D.y == 0 ? 1.0f : 0.0f; axis[1] = D.y == 1 ? 1.0f : 0.0f; axis[2] = D.y == 2 ? 1.0f : 0.0f; }
      else {
        float m[9]; quat2mat(m, xq + 4 * b);
        const int k = D.y - 3;
        axis[0] = sel3(m[0], m[1], m[2], k); axis[1] = sel3(m[3], m[4], m[5], k); axis[2] = sel3(m[6], m[7], m[8], k);
        anchor[0] = xp[3 * b]; anchor[1] = xp[3 * b + 1]; anchor[2] = xp[3 * b + 2];
        kind = 1;
      }
    } else {
      const int4 B = A.M.body[b];
      const int p = B.x;
      float mat[9], pos[3], quat[4], t[3];
      quat2mat(mat, xq + 4 * p); rotvec(t, mat, A.M.body_pos + 3 * b);
      pos[0] = xp[3 * p] + t[0]; pos[1] = xp[3 * p + 1] + t[1]; pos[2] = xp[3 * p + 2] + t[2];
      mulquat(quat, xq + 4 * p, A.M.body_quat + 4 * b);
      for (int j = B.y; j <= D.w; j++) {
        const int2 J = A.M.jnt[j];
        const int jt = J.x, qa = J.y;
        float vec[3], anc[3], ax[3];
        quat2mat(mat, quat);
        rotvec(vec, mat, A.M.jnt_pos + 3 * j);
        anc[0] = pos[0] + vec[0]; anc[1] = pos[1] + vec[1]; anc[2] = pos[2] + vec[2];
        rotvec(ax, mat, A.M.jnt_axis + 3 * j);
        float ql[4] = {1.0f, 0.0f, 0.0f, 0.0f};
        if (jt == MJH_JNT_BALL) { ql[0] = qpos[qa]; ql[1] = qpos[qa + 1]; ql[2] = qpos[qa + 2]; ql[3] = qpos[qa + 3]; normalize4(ql); }
        else if (jt == MJH_JNT_HINGE) axisangle2quat(ql, A.M.jnt_axis + 3 * j, qpos[qa] - A.M.qpos0[qa]);
        if (j == D.w) {
          if (jt == MJH_JNT_BALL) {      // the body's axes after the ball's rotation, through the joint anchor
            float r[4]; mulquat(r, quat, ql); quat2mat(mat, r);
            ax[0] = sel3(mat[0], mat[1], mat[2], D.y); ax[1] = sel3(mat[3], mat[4], mat[5], D.y); ax[2] = sel3(mat[6], mat[7], mat[8], D.y);
          }
          axis[0] = ax[0]; axis[1] = ax[1]; axis[2] = ax[2];
          if (jt != MJH_JNT_SLIDE) { anchor[0] = anc[0]; anchor[1] = anc[1]; anchor[2] = anc[2]; kind = 1; }
          break;
        }
        if (jt == MJH_JNT_SLIDE) {
          const float dq = qpos[qa] - A.M.qpos0[qa];
          pos[0] += ax[0] * dq; pos[1] += ax[1] * dq; pos[2] += ax[2] * dq;
        } else if (jt == MJH_JNT_BALL || jt == MJH_JNT_HINGE) {
          float r[4]; mulquat(r, quat, ql);
          quat[0] = r[0]; quat[1] = r[1]; quat[2] = r[2]; quat[3] = r[3];
          quat2mat(mat, quat); rotvec(vec, mat, A.M.jnt_pos + 3 * j);
          pos[0] = anc[0] - vec[0]; pos[1] = anc[1] - vec[1]; pos[2] = anc[2] - vec[2];
        }
      }
    }
    s_stage[d] = axis[0]; s_stage[nv + d] = axis[1]; s_stage[2 * nv + d] = axis[2];
    s_stage[3 * nv + d] = anchor[0]; s_stage[4 * nv + d] = anchor[1]; s_stage[5 * nv + d] = anchor[2];
    s_stage[6 * nv + d] = __int_as_float(kind); s_stage[7 * nv + d] = qvel[d];
  }
  __syncthreads();
  for (int f = 0; f < A.nframe; f++) {
    const FrameRec R = A.frames[f];
    const int body = U(R.body), site = U(R.site);
    const size_t o = (size_t)row * (size_t)A.nframe + (size_t)f;
    float p[3], q[4], v[3], w[3];
    frame_pose(A, xp, xq, body, site, p, q);
    frame_twist(A, s_stage, lane, body, p, A.jac ? A.jac + o * 6 * (size_t)nv : nullptr, v, w);
    if (U(R.ref)) {
      // relative to the ref frame, in its axes: pos = R^T (p - pr), quat = qr^-1 q, linvel = R^T (v - vr - wr x (p - pr)), angvel = R^T (w - wr)
      float pr[3], qr[4], vr[3], wr[3], m[9], dp[3], c[3], t[3], qc[4], qq[4];
      const int rbody = U(R.rbody), rsite = U(R.rsite);
      frame_pose(A, xp, xq, rbody, rsite, pr, qr);
      frame_twist(A, s_stage, lane, rbody, pr, nullptr, vr, wr);
      quat2mat(m, qr);
      dp[0] = p[0] - pr[0]; dp[1] = p[1] - pr[1]; dp[2] = p[2] - pr[2];
      cross3(c, wr, dp);
      t[0] = v[0] - vr[0] - c[0]; t[1] = v[1] - vr[1] - c[1]; t[2] = v[2] - vr[2] - c[2];
      rotvecT(v, m, t);
      t[0] = w[0] - wr[0]; t[1] = w[1] - wr[1]; t[2] = w[2] - wr[2];
      rotvecT(w, m, t);
      rotvecT(p, m, dp);
      qc[0] = qr[0]; qc[1] = -qr[1]; qc[2] = -qr[2]; qc[3] = -qr[3];
      mulquat(qq, qc, q);
      q[0] = qq[0]; q[1] = qq[1]; q[2] = qq[2]; q[3] = qq[3];
    } else if (U(R.local)) {
      float m[9]; quat2mat(m, q);
      rotvecT(v, m, v); rotvecT(w, m, w);
    }
    if (lane == 0) {
      float* out = A.state + o * FR_STATE;
      out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
      out[3] = q[0]; out[4] = q[1]; out[5] = q[2]; out[6] = q[3];
      out[7] = v[0]; out[8] = v[1]; out[9] = v[2];
      out[10] = w[0]; out[11] = w[1]; out[12] = w[2];
    }
  }
}

hipError_t mjh_launch_frame_state(hipStream_t st, const FrameArgs& A) {
  if (A.n <= 0 || A.nframe <= 0 || A.M.nbody <= 0 || A.M.nw <= 0 || !A.xpos || !A.xquat || !A.qpos || !A.qvel || !A.frames || !A.state) return hipErrorInvalidValue;
  if (A.M.nv > 0 && (!A.M.dof || !A.M.body || !A.M.chain)) return hipErrorInvalidValue;
  const size_t lds = frame_lds_bytes(A.M.nv);
  if (lds > FR_LDS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mjh_frame_state_kernel, dim3((unsigned)A.n), dim3(64), lds, st, A);
  return hipGetLastError();
}
