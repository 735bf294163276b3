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

static __device__ __forceinline__ float uniform(float x) { return ray_float(ray_uniform(ray_bits(x))); }

// One workgroup (one wavefront) per (env, tile of TH x TW cells), one cell per lane: row lane >> tw_log, column lane & (TW - 1); the
// shape is a launch argument (scan_tile_shape), the same for every wave.  Staging, compaction and the walk are depth.hip's: the env's
// geom records are staged RAY_PASS geoms per pass, only the visible geoms whose bounding sphere touches the tile's cylinder reach LDS,
// in ascending geom id (so ties break as in ray.hip).  Planes and height fields are never culled.  cull = 0 skips the cylinder test
// only: the images are the same bits.  exclude_tree is a test of this kernel's own after ray_verdict: a geom whose body has the
// excluded root is dropped like an invisible one.
// TRI and amdgpu_num_sgpr(96): as mjh_scan_kernel (DESIGN.md section 4g has the figures).
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) __attribute__((amdgpu_num_sgpr(96))) void mjh_heightscan_kernel(const HScanArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const RayScene& W = A.W;
  const int lane = (int)threadIdx.x;
  const int tw_log = A.tw_log, TW = 1 << tw_log, TH = RAY_TILE >> tw_log;
  const int tx = (A.width + TW - 1) >> tw_log, ty = (A.height + TH - 1) >> (6 - tw_log), ntile = tx * ty;
  const int row = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - row * ntile;
  if (row >= W.n) return;
  const int env = W.env0 + row;
  const int trow = tile / tx, tcol = tile - trow * tx;
  const int i0 = trow * TH, j0 = tcol << tw_log;
  const int pi = i0 + (lane >> tw_log), pj = j0 + (lane & (TW - 1));
  const bool live = pi < A.height && pj < A.width;

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
  hscan_tile_bound(i0, min(TH, A.height - i0), j0, min(TW, A.width - j0), A.width, A.height, A.ox, A.oy, A.hx, A.hy, tcx, tcy, radius);
#pragma unroll
  for (int k = 0; k < 3; k++) ax[k] = uniform(o[k] + G[3*k] * tcx + G[3*k+1] * tcy + G[3*k+2] * A.above);
  radius = uniform(radius);

  const unsigned slotmask = W.slot_mask ? W.slot_mask[env] : 0u;
  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;

  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < W.ngeom; base += RAY_PASS) {
    __syncthreads();
    const int g = base + lane;
    // stage geom g of this env: the verdict first (type, body, bounding sphere), then only a survivor's record is read and stored
    int4 gi = make_int4(-1, 0, 0, 0);
    float c[3] = {0.0f, 0.0f, 0.0f}, s[3] = {0.0f, 0.0f, 0.0f}, rb = 0.0f;
    bool keep = false;
    if (g < W.ngeom) {
      gi = W.ginfo[g];
      const float* gp = W.gpos + ((size_t)row * W.ngeom + g) * 3;
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = gp[k];
#pragma unroll
      for (int k = 0; k < 3; k++) s[k] = gsize[3*g + k];
      keep = ray_verdict<TRI>(W, gi, s, slotmask, rb, &A.T) >= 0;
      if (keep && A.root_ex >= 0) keep = A.rootid[gi.y] != A.root_ex;      // the sensor's whole kinematic tree is hidden
      if (keep && A.cull && gi.x >= MJH_GEOM_SPHERE) keep = hscan_tile_keep(ax, v, radius, c, rb);      // planes and height fields are never culled
    }
    const unsigned long long kept = __ballot(keep);
    if (keep) {      // the survivors in ascending geom id: record `number of survivors in the lanes below`
      const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
      ray_store(s_rec + slot * RAY_REC, c, W.gmat + ((size_t)row * W.ngeom + g) * 9, s, rb, gi.x, gi.w, g);
    }
    __syncthreads();
    ray_walk<false, TRI>(W, s_rec, __popcll(kept), p, v, vv, valid, best, bestg, &A.T);
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
  const int TW = 1 << A.tw_log, TH = RAY_TILE >> A.tw_log;
  const long long tx = (A.width + TW - 1) / TW, ty = (A.height + TH - 1) / TH, blocks = tx * ty * (long long)A.W.n;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (A.T.mesh) hipLaunchKernelGGL(mjh_heightscan_kernel<true>, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  else hipLaunchKernelGGL(mjh_heightscan_kernel<false>, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  return hipGetLastError();
}
