// frame_acc.hip — mjh_frame_accel_kernel: classical acceleration (J qacc + Jdot qvel) and bias (Jdot qvel) of selected bodies and sites of
// every env, from the body poses the position-stage launch exported (PH_FKONLY with XF_BODY), the envs' qpos / qvel and the engine's qacc
// of the last solve.  A translation unit of its own: no compiled code of frame.hip or of the step kernels is touched.  Stream-ordered behind
// the steps queued so far; nothing of the envs' state is written.  gfx950 only.
#include <hip/hip_runtime.h>

// No contraction anywhere in this unit, the helpers of dev_math.h included: every product and sum is rounded as written, so that a frame's
// numbers are a function of the env's state and the frame alone — whichever call, position in the frame table or output selection the
// compiler specialises a copy of the walk for.
#pragma clang fp contract(off)

#include "../../include/mjhip.h"
#include "dev_frame.h"
#include "dev_math.h"

#define U(x) __builtin_amdgcn_readfirstlane(x)      // a wave-uniform integer, kept in a scalar register

// world pose of (body, site), as frame.hip forms it: the exported body pose; a site adds its offset as the step kernel's site frames do
static __device__ __forceinline__ void facc_pose(const FrameModel& M, const float* xp, const float* xq, int body, int site, float p[3], float q[4]) {
  const float* bp = xp + 3 * body; const float* bq = xq + 4 * body;
  if (site < 0) {
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = bp[k];
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = bq[k];
  } else {
    float m[9], t[3];
    quat2mat(m, bq); rotvec(t, m, M.site_pos + 3 * site);
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = bp[k] + t[k];
    mulquat(q, bq, M.site_quat + 4 * site);
  }
}

// Stage 1 of a dof, as frame.hip's stage loop forms it (the same operations in the same order, so the columns are the Jacobian's of
// mjh_frame_state): kind (0 translation, 1 rotation), world axis and world anchor from the PARENT's exported pose, body_pos / body_quat and
// the body's own joints up to the dof's own, in mj_kinematics' order (a free joint's from the body's own pose).
static __device__ __forceinline__ int facc_column(const FrameModel& M, const float* xp, const float* xq, const float* qpos, const int4 D,
                                                  float axis[3], float anchor[3]) {
  const int b = D.z;
  int kind = 0;
  axis[0] = 0.0f; axis[1] = 0.0f; axis[2] = 0.0f; anchor[0] = 0.0f; anchor[1] = 0.0f; anchor[2] = 0.0f;
  if (D.x == MJH_JNT_FREE) {
    if (D.y < 3) { axis[0] = D.y == 0 ? 1.0f : 0.0f; axis[1] = D.y == 1 ? 1.0f : 0.0f; axis[2] = D.y == 2 ? 1.0f : 0.0f; }
    else {
      float m[9]; quat2mat(m, xq + 4 * b);
      const int k = D.y - 3;
      axis[0] = sel3(m[0], m[1], m[2], k); axis[1] = sel3(m[3], m[4], m[5], k); axis[2] = sel3(m[6], m[7], m[8], k);
      anchor[0] = xp[3 * b]; anchor[1] = xp[3 * b + 1]; anchor[2] = xp[3 * b + 2];
      kind = 1;
    }
    return kind;
  }
  const int4 B = M.body[b];
  const int p = B.x;
  float mat[9], pos[3], quat[4], t[3];
  quat2mat(mat, xq + 4 * p); rotvec(t, mat, M.body_pos + 3 * b);
  pos[0] = xp[3 * p] + t[0]; pos[1] = xp[3 * p + 1] + t[1]; pos[2] = xp[3 * p + 2] + t[2];
  mulquat(quat, xq + 4 * p, M.body_quat + 4 * b);
  for (int j = B.y; j <= D.w; j++) {
    const int2 J = M.jnt[j];
    const int jt = J.x, qa = J.y;
    float vec[3], anc[3], ax[3];
    quat2mat(mat, quat);
    rotvec(vec, mat, M.jnt_pos + 3 * j);
    anc[0] = pos[0] + vec[0]; anc[1] = pos[1] + vec[1]; anc[2] = pos[2] + vec[2];
    rotvec(ax, mat, M.jnt_axis + 3 * j);
    float ql[4] = {1.0f, 0.0f, 0.0f, 0.0f};
    if (jt == MJH_JNT_BALL) { ql[0] = qpos[qa]; ql[1] = qpos[qa + 1]; ql[2] = qpos[qa + 2]; ql[3] = qpos[qa + 3]; normalize4(ql); }
    else if (jt == MJH_JNT_HINGE) axisangle2quat(ql, M.jnt_axis + 3 * j, qpos[qa] - M.qpos0[qa]);
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
      const float dq = qpos[qa] - M.qpos0[qa];
      pos[0] += ax[0] * dq; pos[1] += ax[1] * dq; pos[2] += ax[2] * dq;
    } else if (jt == MJH_JNT_BALL || jt == MJH_JNT_HINGE) {
      float r[4]; mulquat(r, quat, ql);
      quat[0] = r[0]; quat[1] = r[1]; quat[2] = r[2]; quat[3] = r[3];
      quat2mat(mat, quat); rotvec(vec, mat, M.jnt_pos + 3 * j);
      pos[0] = anc[0] - vec[0]; pos[1] = anc[1] - vec[1]; pos[2] = anc[2] - vec[2];
    }
  }
  return kind;
}

// the bit of dof d = d0 + lane in the chain mask mk of a body (wave-uniform words, as frame.hip's walk reads them)
static __device__ __forceinline__ bool facc_in_chain(const unsigned* mk, int nw, int nv, int d0, int lane) {
  const int wi = d0 >> 5;
  const unsigned lo = U(mk[wi]), hi = wi + 1 < nw ? U(mk[wi + 1]) : 0u;
  return d0 + lane < nv && (((lane < 32 ? lo : hi) >> (lane & 31)) & 1u);
}

// One workgroup (one wavefront) per env, lanes = dofs.  LDS: FRA_STAGE words per dof, one array per word (conflict-free over d) —
//   0-2 world axis a_d, 3-5 world anchor r_d, 6 kind, 7 qvel_d, 8 qacc_d          (stage 1, as mjh_frame_state_kernel plus qacc)
//   9-11 w_pre(d): angular velocity of the frame the joint of d is mounted in; 12-14 rdot_d: velocity of the anchor     (stage 2)
// Stage 2, once per env and independent of the frames: over the chain dofs e < d of d's own body, in ascending e,
//   w_pre += a_e qvel_e   for rotational e in front of d's JOINT (hinge / slide: e < d; ball / free: e before the joint's first rotational
//                         dof — the joint's three columns turn with the body's full angular velocity, and their own terms cancel in the sum
//                         over the three: (w_pre + w_own) x w_own = w_pre x w_own)
//   rdot  += c_e(r_d) qvel_e,   c_e(x) = a_e (translation), a_e x (x - r_e) (rotation; exactly zero for the dofs of d's own ball / free
//                         joint, whose anchors are the same bits; a free joint's translational dofs move its anchor)
// Walk, wave-uniform over the frames: v_p = jacp qvel first (the sum of mjh_frame_state's twist), then per lane in the frame's chain
//   translation:  cdot = (w_pre x a_d, 0)
//   rotation:     cdot = ((w_pre x a_d) x (p - r_d) + a_d x (v_p - rdot_d),  w_pre x a_d)
// bias += cdot qvel_d and direct += c_d qacc_d over d = lane, lane + 64, .. in ascending order, one butterfly per sum, acc = direct + bias.
__global__ __launch_bounds__(64) void mjh_frame_accel_kernel(const FrameAccArgs A) {
  extern __shared__ float s[];
  const int lane = (int)threadIdx.x, row = (int)blockIdx.x;
  if (row >= A.n) return;
  const int env = A.env0 + row, nv = A.M.nv, nb = A.M.nbody, nw = A.M.nw;
  const float* const xp = A.xpos + (size_t)row * 3 * nb;
  const float* const xq = A.xquat + (size_t)row * 4 * nb;
  const float* const qpos = A.qpos + (size_t)env * A.nqp;
  const float* const qvel = A.qvel + (size_t)env * A.nvp;
  const float* const qacc = A.qacc + (size_t)env * A.nvp;
  for (int d = lane; d < nv; d += 64) {
    float axis[3], anchor[3];
    const int kind = facc_column(A.M, xp, xq, qpos, A.M.dof[d], axis, anchor);
    s[d] = axis[0]; s[nv + d] = axis[1]; s[2 * nv + d] = axis[2];
    s[3 * nv + d] = anchor[0]; s[4 * nv + d] = anchor[1]; s[5 * nv + d] = anchor[2];
    s[6 * nv + d] = __int_as_float(kind); s[7 * nv + d] = qvel[d]; s[8 * nv + d] = qacc[d];
  }
  __syncthreads();
  for (int d = lane; d < nv; d += 64) {
    const int4 D = A.M.dof[d];
    // the first dof that is not in front of d's joint
    const int wlim = D.x == MJH_JNT_BALL ? d - D.y : (D.x == MJH_JNT_FREE ? d - D.y + 3 : d);
    const unsigned* mk = A.M.chain + (size_t)D.z * nw;
    const float rd[3] = {s[3 * nv + d], s[4 * nv + d], s[5 * nv + d]};
    float wp[3] = {0.0f, 0.0f, 0.0f}, rv[3] = {0.0f, 0.0f, 0.0f};
    for (int wi = 0; wi * 32 < d; wi++) {
      unsigned bits = mk[wi];
      if ((wi + 1) * 32 > d) bits &= (1u << (d - wi * 32)) - 1u;      // e < d
      while (bits) {
        const int e = wi * 32 + __ffs(bits) - 1;
        bits &= bits - 1u;
        const float ae[3] = {s[e], s[nv + e], s[2 * nv + e]};
        const float qe = s[7 * nv + e];
        if (__float_as_int(s[6 * nv + e])) {
          const float r[3] = {rd[0] - s[3 * nv + e], rd[1] - s[4 * nv + e], rd[2] - s[5 * nv + e]};
          float c[3];
          cross3(c, ae, r);
          rv[0] += c[0] * qe; rv[1] += c[1] * qe; rv[2] += c[2] * qe;
          if (e < wlim) { wp[0] += ae[0] * qe; wp[1] += ae[1] * qe; wp[2] += ae[2] * qe; }
        } else { rv[0] += ae[0] * qe; rv[1] += ae[1] * qe; rv[2] += ae[2] * qe; }
      }
    }
    s[9 * nv + d] = wp[0]; s[10 * nv + d] = wp[1]; s[11 * nv + d] = wp[2];
    s[12 * nv + d] = rv[0]; s[13 * nv + d] = rv[1]; s[14 * nv + d] = rv[2];
  }
  __syncthreads();
  for (int f = 0; f < A.nframe; f++) {
    const FrameRec R = A.frames[f];
    const int body = U(R.body), site = U(R.site);
    const unsigned* mk = A.M.chain + (size_t)body * nw;
    float p[3], q[4];
    facc_pose(A.M, xp, xq, body, site, p, q);
    // the point's world velocity: mjh_frame_state's linvel sum
    float vp[3] = {0.0f, 0.0f, 0.0f};
    for (int d0 = 0; d0 < nv; d0 += 64) {
      const int d = d0 + lane;
      float c[3] = {0.0f, 0.0f, 0.0f};
      float qv = 0.0f;
      if (facc_in_chain(mk, nw, nv, d0, lane)) {
        const float ax[3] = {s[d], s[nv + d], s[2 * nv + d]};
        if (__float_as_int(s[6 * nv + d])) {
          const float r[3] = {p[0] - s[3 * nv + d], p[1] - s[4 * nv + d], p[2] - s[5 * nv + d]};
          cross3(c, ax, r);
        } else { c[0] = ax[0]; c[1] = ax[1]; c[2] = ax[2]; }
        qv = s[7 * nv + d];
      }
#pragma unroll
      for (int k = 0; k < 3; k++) vp[k] += c[k] * qv;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) vp[k] = frame_wave_sum(vp[k]);
    float bias[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, dir[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int d0 = 0; d0 < nv; d0 += 64) {
      const int d = d0 + lane;
      float c[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, cd[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
      float qv = 0.0f, qa = 0.0f;
      if (facc_in_chain(mk, nw, nv, d0, lane)) {
        const float ax[3] = {s[d], s[nv + d], s[2 * nv + d]};
        const float wp[3] = {s[9 * nv + d], s[10 * nv + d], s[11 * nv + d]};
        float da[3];
        cross3(da, wp, ax);
        if (__float_as_int(s[6 * nv + d])) {
          const float r[3] = {p[0] - s[3 * nv + d], p[1] - s[4 * nv + d], p[2] - s[5 * nv + d]};
          const float u[3] = {vp[0] - s[12 * nv + d], vp[1] - s[13 * nv + d], vp[2] - s[14 * nv + d]};
          float t1[3], t2[3];
          cross3(c, ax, r);
          c[3] = ax[0]; c[4] = ax[1]; c[5] = ax[2];
          cross3(t1, da, r); cross3(t2, ax, u);
          cd[0] = t1[0] + t2[0]; cd[1] = t1[1] + t2[1]; cd[2] = t1[2] + t2[2];
          cd[3] = da[0]; cd[4] = da[1]; cd[5] = da[2];
        } else {
          c[0] = ax[0]; c[1] = ax[1]; c[2] = ax[2];
          cd[0] = da[0]; cd[1] = da[1]; cd[2] = da[2];
        }
        qv = s[7 * nv + d]; qa = s[8 * nv + d];
      }
#pragma unroll
      for (int r = 0; r < 6; r++) { bias[r] += cd[r] * qv; dir[r] += c[r] * qa; }
    }
    float acc[6];
#pragma unroll
    for (int r = 0; r < 6; r++) { bias[r] = frame_wave_sum(bias[r]); dir[r] = frame_wave_sum(dir[r]); acc[r] = dir[r] + bias[r]; }
    if (U(R.proper)) { acc[0] = acc[0] - A.gravity[0]; acc[1] = acc[1] - A.gravity[1]; acc[2] = acc[2] - A.gravity[2]; }
    if (U(R.local)) {
      float m[9]; quat2mat(m, q);
      rotvecT(acc, m, acc); rotvecT(acc + 3, m, acc + 3);
    }
    if (lane == 0) {
      const size_t o = ((size_t)row * (size_t)A.nframe + (size_t)f) * FRA_OUT;
#pragma unroll
      for (int r = 0; r < 6; r++) A.acc[o + r] = acc[r];
      if (A.bias) {
#pragma unroll
        for (int r = 0; r < 6; r++) A.bias[o + r] = bias[r];
      }
    }
  }
}

hipError_t mjh_launch_frame_accel(hipStream_t st, const FrameAccArgs& A) {
  if (A.n <= 0 || A.nframe <= 0 || A.M.nbody <= 0 || A.M.nw <= 0 || !A.xpos || !A.xquat || !A.qpos || !A.qvel || !A.qacc || !A.frames || !A.acc) return hipErrorInvalidValue;
  if (A.M.nv > 0 && (!A.M.dof || !A.M.body || !A.M.chain)) return hipErrorInvalidValue;
  const size_t lds = frame_acc_lds_bytes(A.M.nv);
  if (lds > FR_LDS_MAX) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mjh_frame_accel_kernel, dim3((unsigned)A.n), dim3(64), lds, st, A);
  return hipGetLastError();
}
