// dev_depth.h — depth images (mjh_depth / mjh_depth_device): what the depth kernel (depth.hip) adds to the scene of dev_ray.h — its
// launch descriptor, the pixel-direction function and the sphere-cone predicate of the tile cull.  The functions are __host__ __device__:
// tests/depth_host builds them for the CPU and checks the very code the kernel runs.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_ray.h"

#define DEPTH_TILE_LOG 3
#define DEPTH_TILE (1 << DEPTH_TILE_LOG)   // a wavefront renders a DEPTH_TILE x DEPTH_TILE pixel tile: column lane & 7, row lane >> 3

// The tile map of the image kernels (depth, shade, light, texture: tw_log = DEPTH_TILE_LOG; scan, heightscan: a launch argument,
// dev_scan.h: scan_tile_shape): a width x height image is cut into tiles of TH x TW lanes, TW = 1 << tw_log, TH = RAY_TILE >> tw_log, a
// lane's row in its tile is lane >> tw_log and its column lane & (TW - 1); one workgroup per (env row, tile), the tiles of an env row by
// row.  tile_blocks: the workgroups of a launch over n envs.
static __host__ __device__ __forceinline__ int tile_columns(int width, int tw_log) { return (width + (1 << tw_log) - 1) >> tw_log; }
static __host__ __device__ __forceinline__ int tile_rows(int height, int tw_log) { return (height + (RAY_TILE >> tw_log) - 1) >> (6 - tw_log); }
static inline long long tile_blocks(int width, int height, int tw_log, int n) {
  return (long long)tile_columns(width, tw_log) * (long long)tile_rows(height, tw_log) * (long long)n;
}
// what workgroup `block` of env row `row` and its lane `lane` hold: the tile's first pixel (i0, j0) and its extent inside the image
// (ni, nj), the lane's pixel (pi, pj) and whether it lies inside the image (live)
struct TileMap { int i0, j0, ni, nj, pi, pj; bool live; };

struct DepthArgs {
  RayScene W;
  float* depth; int* geomid;       // [n][height][width]; geomid may be null
  int width, height;
  int range, cull;                 // range: report the distance from the camera origin, not the depth; cull: the tile-cone test
  int cam_body; float cam_pos[3], cam_quat[4];   // camera frame in its body
  float scale;                     // tan(fovy / 2) / height: half the side of a (square) pixel on the plane z = -1
  RayTris T;
};

hipError_t mjh_launch_depth(hipStream_t st, const DepthArgs& A);   // depth.hip

#ifdef __HIPCC__
// Integers only; with a literal tw_log they fold.  Two steps, because the kernel tests `row >= n` (a workgroup beyond the launch's env
// rows returns at once) between them: with the test behind tile_map's division the kernel's first loads wait for it (HISTORY.md).
static __device__ __forceinline__ int tile_row(int block, int width, int height, int tw_log) {
  return block / (tile_columns(width, tw_log) * tile_rows(height, tw_log));
}
static __device__ __forceinline__ TileMap tile_map(int block, int row, int lane, int width, int height, int tw_log) {
  const int TW = 1 << tw_log, TH = RAY_TILE >> tw_log;
  const int tx = tile_columns(width, tw_log), ntile = tx * tile_rows(height, tw_log);
  const int tile = block - row * ntile, trow = tile / tx, tcol = tile - trow * tx;
  TileMap t;
  t.i0 = trow * TH; t.j0 = tcol << tw_log;
  t.ni = min(TH, height - t.i0); t.nj = min(TW, width - t.j0);
  t.pi = t.i0 + (lane >> tw_log); t.pj = t.j0 + (lane & (TW - 1));
  t.live = t.pi < height && t.pj < width;
  return t;
}

// the ray through the centre of pixel (row i from the top, column j from the left) in the camera frame (looks along -z, +x right, +y up):
// d = (a t (2 (j + 1/2) / W - 1), t (1 - 2 (i + 1/2) / H), -1) with a = W / H, so both factors are t / H = scale.  The integer
// numerators are exact in fp32: each component carries one rounding besides that of `scale`.
RDEV void depth_pixel_dir(int i, int j, int width, int height, float scale, float* d) {
  d[0] = scale * (float)(2 * j + 1 - width);
  d[1] = scale * (float)(height - 2 * i - 1);
  d[2] = -1.0f;
}

// the cone of the tile of pixels [i0, i0 + ni) x [j0, j0 + nj), camera frame, apex at the camera origin: the unit axis goes through the
// centre of the tile's footprint on the plane z = -1; cosA / sinA of the half-angle that covers the footprint's four outer corners
// (below 90 degrees: every corner has z = -1)
RDEV void depth_tile_cone(int i0, int j0, int ni, int nj, int width, int height, float scale, float* axis, float& cosA, float& sinA) {
  const float x0 = scale * (float)(2 * j0 - width), x1 = scale * (float)(2 * (j0 + nj) - width);
  const float y0 = scale * (float)(height - 2 * i0), y1 = scale * (float)(height - 2 * (i0 + ni));
  const float cx = 0.5f * (x0 + x1), cy = 0.5f * (y0 + y1);
  const float inv = 1.0f / sqrtf(cx*cx + cy*cy + 1.0f);
  axis[0] = cx * inv; axis[1] = cy * inv; axis[2] = -inv;
  cosA = 1.0f; sinA = 0.0f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float x = (k & 1) ? x1 : x0, y = (k & 2) ? y1 : y0;
    const float il = 1.0f / sqrtf(x*x + y*y + 1.0f);
    // sine from the cross product: 1 - cos^2 would cancel for the narrow cone of a small tile
    const float u = y * axis[2] + axis[1], v = -axis[0] - x * axis[2], w = x * axis[1] - y * axis[0];
    cosA = fminf(cosA, (x * axis[0] + y * axis[1] - axis[2]) * il);
    sinA = fmaxf(sinA, sqrtf(u*u + v*v + w*w) * il);
  }
}

// does the sphere (centre c relative to the cone's apex, radius r) touch the solid cone (unit axis, half-angle A below 90 degrees), or
// hold the apex?  Conservative: true whenever a ray from the apex inside the cone meets the sphere.  With h = c . axis and
// q = |c x axis| the centre lies q cosA - h sinA outside the cone's surface (negative: inside); a sphere wholly behind the plane
// through the apex cannot touch a cone narrower than a half-space.  The slack covers the fp32 roundings (a few 1e-7 (|c| + r)).
RDEV bool depth_cone_keep(const float* axis, float cosA, float sinA, const float* c, float r) {
  const float cc = c[0]*c[0] + c[1]*c[1] + c[2]*c[2];
  if (cc <= r * r) return true;      // the camera sits inside the sphere
  const float h = c[0]*axis[0] + c[1]*axis[1] + c[2]*axis[2];
  const float u = c[1]*axis[2] - c[2]*axis[1], v = c[2]*axis[0] - c[0]*axis[2], w = c[0]*axis[1] - c[1]*axis[0];
  const float q = sqrtf(u*u + v*v + w*w);
  const float slack = 2e-5f * (sqrtf(cc) + r);
  return h >= -(r + slack) && q * cosA - h * sinA <= r + slack;
}
#endif
