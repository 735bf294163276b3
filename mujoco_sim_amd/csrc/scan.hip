// scan.hip — mjh_scan_kernel: every env's lidar scan from a site of the model, as range / geom-id images and point clouds.  A
// translation unit of its own: no instance of the step, ray or depth kernels is touched.  The position-stage launch (PH_FKONLY,
// engine.hip: ray_scene) has exported the envs' geom and body poses; this kernel only reads them, the per-env geom sizes, the slot
// masks and the pattern's angle tables, and writes the images.  The beams exist in registers only: a lane's direction is the product
// of its row's and its column's table entries (no device trigonometry), carried into the world by the site's pose in the env.  To the
// shared code of dev_ray.h and the cone test of dev_depth.h it adds the spherical projection, the tile shape and the cone over a tile
// of beams (dev_scan.h).  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_scan.h"

// One workgroup (one wavefront) per (env, tile of TH x TW beams), one beam per lane: row lane >> tw_log, column lane & (TW - 1)
// (dev_depth.h: tile_map); the shape is a launch argument (scan_tile_shape), the same for every wave.  The env's geom records are
// staged RAY_PASS geoms per pass by ray_stage (dev_ray.h): only the visible geoms whose bounding sphere touches the tile's cone reach
// LDS, compacted in ascending geom id.  Planes and height fields are never culled, and neither is anything in a tile without a cone
// (scan_tile_cone).  cull = 0 skips the cone test only: the images are the same bits.
// TRI and amdgpu_num_sgpr(96): as mjh_depth_kernel — the triangle walk's scalar registers on top of the cone, the scene's and the
// tables' pointers would cost the instance with it a wave per SIMD; capped it keeps the 8 its LDS allows, without scratch (DESIGN.md
// section 4f has the figures).
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) __attribute__((amdgpu_num_sgpr(96))) void mjh_scan_kernel(const ScanArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const RayScene& W = A.W;
  const int lane = (int)threadIdx.x;
  const int row = tile_row((int)blockIdx.x, A.width, A.height, A.tw_log);
  if (row >= W.n) return;
  const TileMap tm = tile_map((int)blockIdx.x, row, lane, A.width, A.height, A.tw_log);
  const int env = W.env0 + row, pi = tm.pi, pj = tm.pj;
  const bool live = tm.live;

  // the sensor's world pose from its body's exported pose, once per env (wave-uniform); without a site the world frame
  float p[3] = {0.0f, 0.0f, 0.0f}, S[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  if (A.site_body >= 0)
    RAY_FRAME(W.xpos + ((size_t)row * W.nbody + A.site_body) * 3, W.xquat + ((size_t)row * W.nbody + A.site_body) * 4, A.site_pos, A.site_quat, p, S);
  // the lane's beam (a dead lane of a partial tile casts the nearest live beam and stores nothing)
  float ds[3], v[3];
  scan_beam_dir(A.tab, A.width, A.height, min(pi, A.height - 1), min(pj, A.width - 1), ds);
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = S[3*k] * ds[0] + S[3*k+1] * ds[1] + S[3*k+2] * ds[2];
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
  const bool valid = vv > 0.0f && vv < 3.0e38f;      // (a non-finite pose sees nothing)
  // the tile's cone in the world frame (wave-uniform): the part of the tile inside the pattern
  float ac[3], axis[3], cosA, sinA;
  const bool cone = scan_tile_cone(A.tab, A.width, A.height, tm.i0, tm.ni, tm.j0, tm.nj, A.az_step, ac, cosA, sinA);
#pragma unroll
  for (int k = 0; k < 3; k++) axis[k] = S[3*k] * ac[0] + S[3*k+1] * ac[1] + S[3*k+2] * ac[2];

  // the sensor origin and the cone are wave-uniform: kept in scalar registers
#pragma unroll
  for (int k = 0; k < 3; k++) { p[k] = uniform(p[k]); axis[k] = uniform(axis[k]); }
  cosA = uniform(cosA); sinA = uniform(sinA);
  const bool cull = A.cull && cone;

  const unsigned slotmask = W.slot_mask ? W.slot_mask[env] : 0u;
  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;

  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < W.ngeom; base += RAY_PASS) {
    const int cnt = ray_stage<TRI>(W, &A.T, s_rec, row, base, lane, slotmask, gsize, [=](bool keep, const int4 gi, const float* c, float rb) {
      if (keep && cull && ray_cullable(gi)) {
        const float rel[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
        keep = depth_cone_keep(axis, cosA, sinA, rel, rb);
      }
      return keep;
    });
    ray_walk<false, TRI>(W, s_rec, cnt, p, v, vv, valid, best, bestg, &A.T);
  }
  // the ray parameter is in units of |v| (1 up to rounding): the range is the Euclidean distance from the sensor origin
  best *= sqrtf(vv);
  if (W.cutoff > 0.0f && best > W.cutoff) bestg = -1;      // the scanner's maximum range: a value beyond it is a miss
  if (bestg < 0) best = -1.0f;
  if (live) {
    const size_t o = ((size_t)row * (size_t)A.height + (size_t)pi) * (size_t)A.width + (size_t)pj;
    A.range[o] = best;
    if (A.geomid) A.geomid[o] = bestg;
    if (A.points) {      // range times the beam in the SENSOR frame; a miss is the origin
      const float r = bestg < 0 ? 0.0f : best;
#pragma unroll
      for (int k = 0; k < 3; k++) A.points[3 * o + k] = r * ds[k];
    }
  }
}

hipError_t mjh_launch_scan(hipStream_t st, const ScanArgs& A) {
  if (A.W.n <= 0 || A.width <= 0 || A.height <= 0 || A.tw_log < 3 || A.tw_log > 6 || !A.tab || !A.range) return hipErrorInvalidValue;
  return RAY_LAUNCH_TRI(mjh_scan_kernel, A.T, tile_blocks(A.width, A.height, A.tw_log, A.W.n), st, A);
}
