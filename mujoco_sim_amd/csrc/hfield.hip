// hfield.hip — translation unit of the mjh_step_kernel instances for models with height-field pairs (HF = true: the collision
// stage adds the prism narrow phase, step_kernel.h) and their launchers.  A unit of its own: the other instances stay in
// engine.hip exactly as they were, and the two units compile side by side.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#define MJH_WINDOW_TU 1        // (step_kernel.h: the helper kernels that are not templates live in engine.hip's unit only)
// two resident waves per SIMD for every instance of this unit: the prism loop keeps the portal state of a prism and the pair's frame
// live beside the collision stage's own registers; at the articulated instances' three-wave budget (168 VGPRs) they spilled
#define MJH_STEP_WAVES 2
#include "step_kernel.h"

// every layout: nr 1 / 2 / 4 LDS-resident, 8 many-body; wpre 0 the whole kernel, 1 / 2 the window chain's assemble-only instances
// (free-body models: diag, nr 1 / 2)
hipError_t mjh_launch_step_hf(hipStream_t st, int nr, bool diag, int wpre, int grid, size_t lds, const DConst* dC, const DState& S,
                              int env0, int nsteps, int ph, int xflags) {
#define MJH_HF(NR, DG, WP) hipLaunchKernelGGL((mjh_step_kernel<NR, DG, true, WP, true>), dim3(grid), dim3(64), lds, st, dC, S, env0, nsteps, ph, xflags)
  if (wpre != 0) {
    if (!diag || nr > 2) return hipErrorInvalidValue;
    if (nr == 1) { if (wpre == 1) MJH_HF(1, true, 1); else MJH_HF(1, true, 2); }
    else { if (wpre == 1) MJH_HF(2, true, 1); else MJH_HF(2, true, 2); }
  } else if (diag) { if (nr == 1) MJH_HF(1, true, 0); else if (nr == 2) MJH_HF(2, true, 0); else if (nr == 4) MJH_HF(4, true, 0); else MJH_HF(8, true, 0); }
  else { if (nr == 1) MJH_HF(1, false, 0); else if (nr == 2) MJH_HF(2, false, 0); else if (nr == 4) MJH_HF(4, false, 0); else MJH_HF(8, false, 0); }
#undef MJH_HF
  return hipGetLastError();
}

// the dynamic-LDS ceiling of every instance above (a launch beyond 64 KB needs the attribute)
hipError_t mjh_step_hf_attributes(size_t lds) {
  hipError_t rc = hipSuccess;
#define MJH_HFA(NR, DG, WP) if (rc == hipSuccess) rc = hipFuncSetAttribute((const void*)mjh_step_kernel<NR, DG, true, WP, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)
  MJH_HFA(1, true, 0); MJH_HFA(2, true, 0); MJH_HFA(4, true, 0); MJH_HFA(8, true, 0);
  MJH_HFA(1, false, 0); MJH_HFA(2, false, 0); MJH_HFA(4, false, 0); MJH_HFA(8, false, 0);
  MJH_HFA(1, true, 1); MJH_HFA(2, true, 1); MJH_HFA(1, true, 2); MJH_HFA(2, true, 2);
#undef MJH_HFA
  return rc;
}
