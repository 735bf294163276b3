// dev_contact.h — per-body contact force from the contact report (contact.hip): the launch descriptor, the staged record and the
// fixed-order sums.  The report itself (records of CREP_STRIDE words per contact, dev_types.h) is written by the step kernel.
#pragma once
#include <hip/hip_runtime.h>

#define CF_REC_WORDS 20      // = CREP_STRIDE (dev_types.h), restated here: this unit includes none of the step kernel's headers
#define CF_FORCE 13
#define CF_GEOM1 17
#define CF_GEOM2 18
#define CF_STAGE 5           // staged per contact: world force (3), body of geom1, body of geom2

struct ContactForceArgs {
  const int* ncon;           // [nenv]
  const float* rec;          // [nenv][maxcon][CF_REC_WORDS]
  const int* geom_bodyid;    // [ngeom]
  const int2* sel;           // [nsel]: body, against (-1: any)
  float* force;              // [n][nsel][3]
  int* count;                // [n][nsel]
  int env0, n, nsel, maxcon, ngeom;
};

// force of contact record r in world axes, on geom2's body: frame^T f (the frame's rows are the normal and the two tangents)
static __device__ __forceinline__ void contact_world_force(const float* r, float w[3]) {
  const float* fr = r + 4; const float* f = r + CF_FORCE;
#pragma unroll
  for (int k = 0; k < 3; k++) w[k] = fr[k] * f[0] + fr[3 + k] * f[1] + fr[6 + k] * f[2];
}

// sum over the wavefront in a fixed order: butterfly over lane distances 32, 16, .. 1 (every lane ends with the same bits)
static __device__ __forceinline__ float contact_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
static __device__ __forceinline__ int contact_wave_sum(int v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}

hipError_t mjh_launch_contact_force(hipStream_t st, const ContactForceArgs& A);
