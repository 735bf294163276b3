// depth.hip — mjh_depth_kernel: every env's view through a camera of the model, as depth / geom-id images.  A translation unit of its
// own: no instance of the step or ray kernels is touched.  The position-stage launch (PH_FKONLY, engine.hip: ray_scene) has exported
// the envs' geom and body poses; this kernel only reads them, the per-env geom sizes and the slot masks, and writes the images.  The
// rays exist in registers only: generated from the camera's intrinsics and its body's pose in the env.  To the shared code of
// dev_ray.h it adds the pixel ray, the tile cone and its test, and `range`.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_depth.h"

// One workgroup (one wavefront) per (env, tile of DEPTH_TILE x DEPTH_TILE pixels), one pixel per lane.  The
// env's geom records are staged RAY_PASS geoms per pass by ray_stage (dev_ray.h): only the visible geoms whose bounding sphere touches
// the tile's cone reach LDS, compacted in ascending geom id, and the walk never meets a record of type -1.  cull = 0 skips the cone test
// only: generation and intersection are the same instructions, so the images are the same bits.
// TRI: the instance for scenes with triangle tables (mesh surface 1; dev_ray.h: ray_walk); the other one is the kernel as it was.
// amdgpu_num_sgpr(96) (no effect on the instance without, which takes 89): with the triangle walk of dev_ray.h (a node and a triangle record in scalar registers on top of the cone and the
// scene's pointers) the kernel would take 106 scalar registers, one wave per SIMD fewer than the 8 its LDS allows.  Capped, six values
// of the prologue (read again once per staging pass and in the epilogue, never in the walk) live in lanes of one VGPR instead: no scratch.
// Derived for the walk as it is: after a change to ray_trimesh / ray_tri look at -Rpass-analysis=kernel-resource-usage and at where the
// v_readlane instructions land again, and drop or move the cap accordingly.
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) __attribute__((amdgpu_num_sgpr(96))) void mjh_depth_kernel(const DepthArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const RayScene& W = A.W;
  const int lane = (int)threadIdx.x;
  // The tile map in this kernel's own text, not tile_row / tile_map of dev_depth.h (the same map; the other five kernels call them), and
  // A.cull read in the predicate, not from a local: with either the prologue is scheduled otherwise, and such builds ran this kernel
  // 0.4 - 1.0 % slower.  As written the unit's instruction sequence is the one it had before the shared pass (HISTORY.md, "One staging pass").
  const int tx = (A.width + DEPTH_TILE - 1) / DEPTH_TILE, ty = (A.height + DEPTH_TILE - 1) / DEPTH_TILE, ntile = tx * ty;
  const int row = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - row * ntile;
  if (row >= W.n) return;
  const int env = W.env0 + row;
  const int trow = tile / tx, tcol = tile - trow * tx;
  const int i0 = trow * DEPTH_TILE, j0 = tcol * DEPTH_TILE;
  const int pi = i0 + (lane >> 3), pj = j0 + (lane & 7);
  const bool live = pi < A.height && pj < A.width;

  // the camera's world pose from its body's exported pose, once per env (wave-uniform)
  float p[3], S[9];
  RAY_FRAME(W.xpos + ((size_t)row * W.nbody + A.cam_body) * 3, W.xquat + ((size_t)row * W.nbody + A.cam_body) * 4, A.cam_pos, A.cam_quat, p, S);
  // the lane's ray (a dead lane of a partial tile casts the ray of the nearest live pixel and stores nothing)
  float dc[3], v[3];
  depth_pixel_dir(min(pi, A.height - 1), min(pj, A.width - 1), A.width, A.height, A.scale, dc);
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = S[3*k] * dc[0] + S[3*k+1] * dc[1] + S[3*k+2] * dc[2];
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
  const bool valid = vv > 0.0f && vv < 3.0e38f;      // (a non-finite pose sees nothing)
  // the tile's cone in the world frame (wave-uniform): the part of the tile inside the image
  float ac[3], axis[3], cosA, sinA;
  depth_tile_cone(i0, j0, min(DEPTH_TILE, A.height - i0), min(DEPTH_TILE, A.width - j0), A.width, A.height, A.scale, ac, cosA, sinA);
#pragma unroll
  for (int k = 0; k < 3; k++) axis[k] = S[3*k] * ac[0] + S[3*k+1] * ac[1] + S[3*k+2] * ac[2];

  // the camera origin and the cone are wave-uniform: kept in scalar registers
#pragma unroll
  for (int k = 0; k < 3; k++) { p[k] = uniform(p[k]); axis[k] = uniform(axis[k]); }
  cosA = uniform(cosA); sinA = uniform(sinA);

  const unsigned slotmask = W.slot_mask ? W.slot_mask[env] : 0u;
  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;

  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < W.ngeom; base += RAY_PASS) {
    const int cnt = ray_stage<TRI>(W, &A.T, s_rec, row, base, lane, slotmask, gsize, [=](bool keep, const int4 gi, const float* c, float rb) {
      if (keep && A.cull && ray_cullable(gi)) {
        const float rel[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
        keep = depth_cone_keep(axis, cosA, sinA, rel, rb);
      }
      return keep;
    });
    ray_walk<false, TRI>(W, s_rec, cnt, p, v, vv, valid, best, bestg, &A.T);
  }
  // dc.z = -1: the ray parameter is the depth along the optical axis; range: the distance from the camera origin
  if (A.range) best *= sqrtf(vv);
  if (W.cutoff > 0.0f && best > W.cutoff) bestg = -1;      // far plane: a value beyond it is a miss
  if (bestg < 0) best = -1.0f;
  if (live) {
    const size_t o = ((size_t)row * (size_t)A.height + (size_t)pi) * (size_t)A.width + (size_t)pj;
    A.depth[o] = best;
    if (A.geomid) A.geomid[o] = bestg;
  }
}

hipError_t mjh_launch_depth(hipStream_t st, const DepthArgs& A) {
  if (A.W.n <= 0 || A.width <= 0 || A.height <= 0) return hipErrorInvalidValue;
  return RAY_LAUNCH_TRI(mjh_depth_kernel, A.T, tile_blocks(A.width, A.height, DEPTH_TILE_LOG, A.W.n), st, A);
}
