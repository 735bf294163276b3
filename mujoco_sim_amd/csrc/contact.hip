// contact.hip — mjh_contact_force_kernel: the net contact force on selected bodies of every env, from the contact report the step kernel
// left (dev_types.h: DReport).  A translation unit of its own: no instance of the step kernels is touched.  It reads the report's records
// and counts, the model's geom_bodyid and the selection table, and writes the sums; stream-ordered behind the steps queued so far.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_contact.h"

// One workgroup (one wavefront) per env.  Stage: lanes = contacts turn their record's contact-frame force into world axes and look up the two
// bodies, once per env (CF_STAGE words per contact in LDS).  Walk: per selected body, every lane adds its contacts c = lane, lane + 64, .. in
// ascending order, +F where the body carries geom2 and -F where it carries geom1 (the record's force acts ON geom2's body), then one butterfly
// over the wavefront.  The order of the additions is a function of the env's own records and the body alone: the sums do not depend on the
// number of envs, the range of the call or the other selected bodies (bitwise).
__global__ __launch_bounds__(64) void mjh_contact_force_kernel(const ContactForceArgs A) {
  extern __shared__ float s_stage[];
  const int lane = (int)threadIdx.x, row = (int)blockIdx.x;
  if (row >= A.n) return;
  const int env = A.env0 + row;
  const int ncon = min(max(A.ncon[env], 0), A.maxcon);
  const float* const rec = A.rec + (size_t)env * (size_t)A.maxcon * CF_REC_WORDS;
  for (int c = lane; c < ncon; c += 64) {
    const float* r = rec + (size_t)c * CF_REC_WORDS;
    float w[3];
    contact_world_force(r, w);
    const int g1 = __float_as_int(r[CF_GEOM1]), g2 = __float_as_int(r[CF_GEOM2]);
    float* p = s_stage + c * CF_STAGE;
    p[0] = w[0]; p[1] = w[1]; p[2] = w[2];
    p[3] = __int_as_float((unsigned)g1 < (unsigned)A.ngeom ? A.geom_bodyid[g1] : -1);
    p[4] = __int_as_float((unsigned)g2 < (unsigned)A.ngeom ? A.geom_bodyid[g2] : -1);
  }
  __syncthreads();
  for (int s = 0; s < A.nsel; s++) {
    const int2 q = A.sel[s];
    float f[3] = {0.0f, 0.0f, 0.0f};
    int cnt = 0;
    for (int c = lane; c < ncon; c += 64) {
      const float* p = s_stage + c * CF_STAGE;
      const int b1 = __float_as_int(p[3]), b2 = __float_as_int(p[4]);
      const bool on2 = b2 == q.x && (q.y < 0 || b1 == q.y), on1 = b1 == q.x && (q.y < 0 || b2 == q.y);
      const float sg = on2 ? 1.0f : (on1 ? -1.0f : 0.0f);
      f[0] += sg * p[0]; f[1] += sg * p[1]; f[2] += sg * p[2];
      cnt += (on1 || on2) ? 1 : 0;
    }
#pragma unroll
    for (int k = 0; k < 3; k++) f[k] = contact_wave_sum(f[k]);
    cnt = contact_wave_sum(cnt);
    if (lane == 0) {
      const size_t o = (size_t)row * (size_t)A.nsel + (size_t)s;
      A.force[3 * o] = f[0]; A.force[3 * o + 1] = f[1]; A.force[3 * o + 2] = f[2];
      if (A.count) A.count[o] = cnt;
    }
  }
}

hipError_t mjh_launch_contact_force(hipStream_t st, const ContactForceArgs& A) {
  if (A.n <= 0 || A.nsel <= 0 || A.maxcon <= 0 || !A.ncon || !A.rec || !A.geom_bodyid || !A.sel || !A.force) return hipErrorInvalidValue;
  const size_t lds = (size_t)A.maxcon * CF_STAGE * sizeof(float);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mjh_contact_force_kernel, dim3((unsigned)A.n), dim3(64), lds, st, A);
  return hipGetLastError();
}
