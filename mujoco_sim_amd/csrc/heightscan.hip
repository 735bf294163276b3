// heightscan.hip — mjh_heightscan_kernel: every env's height scan (elevation map) under a site of the model: a regular grid of parallel
// rays, as range / geom-id images and points in the grid frame.  A translation unit of its own: no instance of the step, ray, depth,
// scan or render kernels is touched.  The position-stage launch (PH_FKONLY, engine.hip: ray_scene) has exported the envs' geom and
// body poses; this kernel only reads them, the per-env geom sizes, the slot masks and the root-id table, and writes the images.  The
// rays exist in registers only: a lane's start point is its cell of the grid, computed from the launch arguments and carried into the
// world by the grid frame of the site's pose in the env; the direction is the same for the whole wave.  To the shared code of dev_ray.h
// and the tile shape of dev_scan.h it adds the orthographic projection, the grid frame and the cylinder over a tile of cells
// (dev_heightscan.h).  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_heightscan.h"

// One workgroup (one wavefront) per (env, tile of TH x TW cells), one cell per lane: row lane >> tw_log, column lane & (TW - 1)
// (dev_depth.h: tile_map); the shape is a launch argument (scan_tile_shape), the same for every wave.  The env's geom records are
// staged RAY_PASS geoms per pass by ray_stage (dev_ray.h): only the visible geoms whose bounding sphere touches the tile's cylinder
// reach LDS, compacted in ascending geom id.  Planes and height fields are never culled.  cull = 0 skips the cylinder test only: the
// images are the same bits.  exclude_tree is a test of this kernel's own after ray_verdict: a geom whose body has the excluded root is
// dropped like an invisible one.
// TRI and amdgpu_num_sgpr(96): as mjh_scan_kernel (DESIGN.md section 4g has the figures).
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) __attribute__((amdgpu_num_sgpr(96))) void mjh_heightscan_kernel(const HScanArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const RayScene& W = A.W;
  const int lane = (int)threadIdx.x;
  const int row = tile_row((int)blockIdx.x, A.width, A.height, A.tw_log);
  if (row >= W.n) return;
  const TileMap tm = tile_map((int)blockIdx.x, row, lane, A.width, A.height, A.tw_log);
  const int env = W.env0 + row, pi = tm.pi, pj = tm.pj;
  const bool live = tm.live;

  // the sensor's world pose from its body's exported pose, once per env (wave-uniform); without a site the world frame
  float o[3] = {0.0f, 0.0f, 0.0f}, S[9] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  if (A.site_body >= 0)
    RAY_FRAME(W.xpos + ((size_t)row * W.nbody + A.site_body) * 3, W.xquat + ((size_t)row * W.nbody + A.site_body) * 4, A.site_pos, A.site_quat, o, S);
  float G[9];
  hscan_grid_frame(A.align, S, G);
  // the lane's cell (a dead lane of a partial tile casts the nearest live cell and stores nothing) and its start point in the world
  float cx, cy;
  hscan_cell(min(pi, A.height - 1), min(pj, A.width - 1), A.width, A.height, A.ox, A.oy, A.hx, A.hy, cx, cy);
  float p[3], v[3];
#pragma unroll
  for (int k = 0; k < 3; k++) p[k] = o[k] + G[3*k] * cx + G[3*k+1] * cy + G[3*k+2] * A.above;
  // the direction -gz is wave-uniform: kept in scalar registers; in YAW and WORLD alignment it is (0, 0, -1) and vv is 1
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = uniform(-G[3*k+2]);
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
  const bool valid = vv > 0.0f && vv < 3.0e38f;      // (a non-finite pose sees nothing)
  // the tile's cylinder in the world frame (wave-uniform): the axis starts at the centre of the live cells on the start plane
  float tcx, tcy, radius, ax[3];
  hscan_tile_bound(tm.i0, tm.ni, tm.j0, tm.nj, A.width, A.height, A.ox, A.oy, A.hx, A.hy, tcx, tcy, radius);
#pragma unroll
  for (int k = 0; k < 3; k++) ax[k] = uniform(o[k] + G[3*k] * tcx + G[3*k+1] * tcy + G[3*k+2] * A.above);
  radius = uniform(radius);

  const unsigned slotmask = W.slot_mask ? W.slot_mask[env] : 0u;
  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;

  const int root_ex = A.root_ex; const int* const rootid = A.rootid; const bool cull = A.cull != 0;
  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < W.ngeom; base += RAY_PASS) {
    const int cnt = ray_stage<TRI>(W, &A.T, s_rec, row, base, lane, slotmask, gsize, [=](bool keep, const int4 gi, const float* c, float rb) {
      if (keep && root_ex >= 0) keep = rootid[gi.y] != root_ex;      // the sensor's whole kinematic tree is hidden, whatever the type
      if (keep && cull && ray_cullable(gi)) keep = hscan_tile_keep(ax, v, radius, c, rb);
      return keep;
    });
    ray_walk<false, TRI>(W, s_rec, cnt, p, v, vv, valid, best, bestg, &A.T);
  }
  // the ray parameter is in units of |v|: exactly 1 in YAW and WORLD alignment, 1 up to rounding in BASE
  if (A.align == MJH_HSCAN_ALIGN_BASE) best *= sqrtf(vv);
  if (W.cutoff > 0.0f && best > W.cutoff) bestg = -1;      // the sensor's maximum range: a value beyond it is a miss
  if (bestg < 0) best = -1.0f;
  if (live) {
    const size_t at = ((size_t)row * (size_t)A.height + (size_t)pi) * (size_t)A.width + (size_t)pj;
    A.range[at] = best;
    if (A.geomid) A.geomid[at] = bestg;
    if (A.points) {      // the cell and the height under it in the GRID frame; a miss is the ray's start point
      A.points[3 * at] = cx; A.points[3 * at + 1] = cy; A.points[3 * at + 2] = A.above - (bestg < 0 ? 0.0f : best);
    }
  }
}

hipError_t mjh_launch_heightscan(hipStream_t st, const HScanArgs& A) {
  if (A.W.n <= 0 || A.width <= 0 || A.height <= 0 || A.tw_log < 3 || A.tw_log > 6 || !A.range || (A.root_ex >= 0 && !A.rootid)) return hipErrorInvalidValue;
  return RAY_LAUNCH_TRI(mjh_heightscan_kernel, A.T, tile_blocks(A.width, A.height, A.tw_log, A.W.n), st, A);
}
