// dev_control.h — the control side of the loop on the device (control.hip): dense fp32 rows of a caller's device buffers <-> the engine's
// per-env rows (commands, PD targets, Cartesian forces, joint state), and the reset of selected envs in one launch.  Every launch is
// enqueued on the stream it is given and waits for nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_types.h"

#define CTL_MAXPART 3

// up to three row blocks moved by one launch: row i of part k is buf[k] + i * width[k] (dense, the caller's) on one side and
// eng[k] + (env0 + i) * stride[k] (the engine's; only `width` floats of a row are touched) on the other.  A part with width 0 is skipped.
struct ControlRowsArgs {
  float* eng[CTL_MAXPART];
  float* buf[CTL_MAXPART];      // (read only by the scatter)
  int stride[CTL_MAXPART], width[CTL_MAXPART];
  int env0, n;
};

// what PH_RESET of the step kernel does to one env (step_kernel.h), for the selected envs of a launch.  Mask form (ids == nullptr): row i is
// env env0 + i, selected when mask == nullptr or mask[i] != 0; qpos / qvel, when given, hold the row a selected env takes ([n][nq], [n][nv]).
// Id-list form: row i is env ids[i] (any order, duplicates write the same values twice).
struct ControlResetArgs {
  const DConst* C;              // model sizes and the contact report's descriptor (C->R)
  DState S;
  const unsigned char* mask;
  const int* ids;
  const float* qpos;
  const float* qvel;
  int env0, n;
};

hipError_t mjh_launch_scatter_rows(hipStream_t st, const ControlRowsArgs& A);   // buf -> eng
hipError_t mjh_launch_gather_rows(hipStream_t st, const ControlRowsArgs& A);    // eng -> buf
hipError_t mjh_launch_reset_rows(hipStream_t st, const ControlResetArgs& A);
