// ray.hip — mjh_ray_kernel: batched ray casting against the geoms of every environment (mj_ray semantics; the laser scans and
// range finders the reference's robots carry).  A translation unit of its own: no instance of the step kernels is touched.
// The position-stage launch (PH_FKONLY, engine.hip: ray_scene) has exported the envs' geom (and body) poses; this kernel only
// reads them, the per-env geom sizes and the slot masks, and writes dist / geomid.  It adds the ray load and the site transform to the
// shared code of dev_ray.h.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_ray.h"

// One workgroup (one wavefront) per (env, tile of RAY_TILE rays), one ray per lane.  The env's geom records are staged into LDS,
// RAY_PASS geoms per pass (one per lane); then every lane walks the records together (dev_ray.h: ray_walk).  Envs are addressed by env
// id (env0 + row of the launch).  TRI: the instance for scenes with triangle tables (mesh surface 1; dev_ray.h: ray_walk).
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) void mjh_ray_kernel(const RayArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const RayScene& W = A.W;
  const int lane = (int)threadIdx.x;
  const int ntile = (A.nray + RAY_TILE - 1) / RAY_TILE;
  const int row = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - row * ntile;
  if (row >= W.n) return;
  const int env = W.env0 + row;
  const int ray = tile * RAY_TILE + lane;
  const bool live = ray < A.nray;
  const size_t ro = ((A.per_env ? (size_t)row * (size_t)A.nray : 0) + (size_t)min(ray, A.nray - 1)) * 3;
  float p[3] = {A.pnt[ro], A.pnt[ro + 1], A.pnt[ro + 2]}, v[3] = {A.vec[ro], A.vec[ro + 1], A.vec[ro + 2]};

  if (A.site_body >= 0) {      // site frame -> world: the site's pose from its body's exported pose, once per env (wave-uniform)
    float sp[3], S[9];
    RAY_FRAME(W.xpos + ((size_t)row * W.nbody + A.site_body) * 3, W.xquat + ((size_t)row * W.nbody + A.site_body) * 4, A.site_pos, A.site_quat, sp, S);
    const float pw[3] = {sp[0] + S[0]*p[0] + S[1]*p[1] + S[2]*p[2], sp[1] + S[3]*p[0] + S[4]*p[1] + S[5]*p[2], sp[2] + S[6]*p[0] + S[7]*p[1] + S[8]*p[2]};
    const float vw[3] = {S[0]*v[0] + S[1]*v[1] + S[2]*v[2], S[3]*v[0] + S[4]*v[1] + S[5]*v[2], S[6]*v[0] + S[7]*v[1] + S[8]*v[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) { p[k] = pw[k]; v[k] = vw[k]; }
  }
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
  const bool valid = vv > 0.0f && vv < 3.0e38f;      // a zero (or non-finite) direction sees nothing
  const unsigned slotmask = W.slot_mask ? W.slot_mask[env] : 0u;
  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;

  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < W.ngeom; base += RAY_PASS) {
    __syncthreads();
    const int g = base + lane;
    if (g < W.ngeom) {       // stage geom g of this env, visible or not: record `lane` of the pass
      const int4 gi = W.ginfo[g];
      const float s[3] = {gsize[3*g], gsize[3*g + 1], gsize[3*g + 2]};
      float rb;
      const int type = ray_verdict<TRI>(W, gi, s, slotmask, rb, &A.T);
      ray_store(s_rec + lane * RAY_REC, W.gpos + ((size_t)row * W.ngeom + g) * 3, W.gmat + ((size_t)row * W.ngeom + g) * 9, s, rb, type, gi.w, g);
    }
    __syncthreads();
    ray_walk<true, TRI>(W, s_rec, min(RAY_PASS, W.ngeom - base), p, v, vv, valid, best, bestg, &A.T);
  }
  if (W.cutoff > 0.0f && best > W.cutoff) bestg = -1;      // rangefinder cutoff: a hit beyond it is a miss
  if (bestg < 0) best = -1.0f;
  if (live) {
    const size_t o = (size_t)row * (size_t)A.nray + (size_t)ray;
    A.dist[o] = best; A.geomid[o] = bestg;
  }
}

hipError_t mjh_launch_ray(hipStream_t st, const RayArgs& A) {
  const long long ntile = ((long long)A.nray + RAY_TILE - 1) / RAY_TILE, blocks = ntile * (long long)A.W.n;
  if (A.W.n <= 0 || A.nray <= 0) return hipErrorInvalidValue;
  return RAY_LAUNCH_TRI(mjh_ray_kernel, A.T, blocks, st, A);
}
