// dev_frame.h — frame states (frame.hip): world pose, twist and Jacobian of bodies and sites from the body poses the position-stage launch
// exported and the envs' qpos / qvel; frame accelerations (frame_acc.hip): classical acceleration and Jdot qvel of the same frames, with
// the engine's qacc.  The launch descriptors, the per-model tables, the staged dof records and the fixed-order sums.
#pragma once
#include <hip/hip_runtime.h>

#define FR_STAGE 8           // staged per dof in LDS: world axis (3), world anchor (3), kind (0 translation, 1 rotation), qvel
#define FR_STATE 13          // per env and frame: pos (3), quat (4, w first), linvel (3), angvel (3)
#define FR_LDS_MAX (64 * 1024)
#define FRA_STAGE 15         // frame accelerations: FR_STAGE, qacc, and per dof the angular velocity in front of its joint (3) and its anchor's velocity (3)
#define FRA_OUT 6            // per env and frame: linear (3), angular (3) — of the acceleration and of the bias Jdot qvel

// a frame of the call as the kernel takes it (ids checked and sites resolved to their bodies on the host)
struct FrameRec {
  int body, site;            // the frame's body; its site or -1
  int rbody, rsite;          // the ref frame's (ref != 0)
  int ref, local;            // 1: pose and twist relative to the ref frame, in its axes; 1: twist in the frame's own axes
  int proper, pad1;          // frame accelerations only — 1: gravity subtracted from the linear acceleration
};

// per-model tables, built on the host at the first call (engine.hip: frame_tables) and shared by every env
struct FrameModel {
  const int4* dof;           // [nv]: joint type, index within the joint, body, joint
  const int4* body;          // [nbody]: parent, first joint, number of joints, mocap id
  const int2* jnt;           // [njnt]: type, qpos address
  const unsigned* chain;     // [nbody][nw]: bit d = dof d moves the body (its own dofs and its ancestors')
  const int* site_body;      // [nsite]
  const float *body_pos, *body_quat, *jnt_pos, *jnt_axis, *qpos0, *site_pos, *site_quat;
  int nv, nbody, njnt, nsite, nw;
};

struct FrameArgs {
  FrameModel M;
  const float *xpos, *xquat; // [n][nbody][3 | 4]: the exported body poses of the env range
  const float *qpos, *qvel;  // [nenv][nqp | nvp]
  const FrameRec* frames;    // [nframe]
  float* state;              // [n][nframe][FR_STATE]
  float* jac;                // [n][nframe][6][nv] or null
  int env0, n, nframe, nqp, nvp;
};

// frame accelerations: the same tables, poses and frame records; qacc is the engine's array of the last solve
struct FrameAccArgs {
  FrameModel M;
  const float *xpos, *xquat; // [n][nbody][3 | 4]: the exported body poses of the env range
  const float *qpos, *qvel, *qacc;  // [nenv][nqp | nvp | nvp]
  const FrameRec* frames;    // [nframe]
  float* acc;                // [n][nframe][FRA_OUT]
  float* bias;               // [n][nframe][FRA_OUT] or null
  float gravity[3];          // what MJH_FRAME_PROPER subtracts (zeros with MJH_DSBL_GRAVITY)
  int env0, n, nframe, nqp, nvp;
};

static inline size_t frame_lds_bytes(int nv) { return (size_t)(nv > 0 ? nv : 1) * FR_STAGE * sizeof(float); }
static inline size_t frame_acc_lds_bytes(int nv) { return (size_t)(nv > 0 ? nv : 1) * FRA_STAGE * sizeof(float); }

#ifdef __HIPCC__
// sum over the wavefront in a fixed order: butterfly over lane distances 32, 16, .. 1 (every lane ends with the same bits)
static __device__ __forceinline__ float frame_wave_sum(float v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
#endif

hipError_t mjh_launch_frame_state(hipStream_t st, const FrameArgs& A);
hipError_t mjh_launch_frame_accel(hipStream_t st, const FrameAccArgs& A);
