// dev_heightscan.h — height scans (mjh_heightscan / mjh_heightscan_device): what the height-scan kernel (heightscan.hip) adds to the scene
// of dev_ray.h and the tile shape of dev_scan.h — its launch descriptor, the argument checks (host), the grid frame of an alignment, the
// cell coordinates and the cylinder test of the tile cull.  The device functions are __host__ __device__: tests/heightscan_host builds
// them for the CPU and checks the very code the kernel runs.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "dev_scan.h"

struct HScanArgs {
  RayScene W;
  float* range; int* geomid; float* points;   // [n][height][width], [n][height][width], [n][height][width][3]; geomid and points may be null
  int width, height;
  int tw_log;                      // tile shape (scan_tile_shape): TW = 1 << tw_log columns, TH = RAY_TILE >> tw_log rows
  int cull;                        // the tile-cylinder test
  int align;                       // MJH_HSCAN_ALIGN_*
  float ox, oy, hx, hy;            // the grid (hscan_cell): offset and HALF the spacing, each the fp64 option rounded to fp32 once
  float above;                     // the rays start this far along +gz from the grid plane
  const int* rootid; int root_ex;  // exclude_tree: body_rootid [nbody] and the root whose bodies no ray sees (root_ex < 0: no such test, rootid unread)
  int site_body; float site_pos[3], site_quat[4];   // sensor frame in its body (site_body < 0: the world frame)
  RayTris T;
};

hipError_t mjh_launch_heightscan(hipStream_t st, const HScanArgs& A);   // heightscan.hip

// ---- the checks on the host (plain C++: the engine and the CPU tests call the same function)

#define HSCAN_FLT_MAX 3.4028234663852886e38

// the checks of a call's arguments against the model's and the engine's sizes (range: the caller's range pointer): null if they are
// good, else what is wrong.  A cell coordinate overflows when the fp32 value of the grid's outermost x or y is not finite, or half a
// spacing is no positive fp32 number.
inline const char* hscan_args_error(int nsite, int nbody, int nenv, int env0, int n, const mjh_heightscan_options& o, const void* range) {
  if (o.site < -1 || o.site >= nsite) return "site id out of range";
  if (o.bodyexclude < -1 || o.bodyexclude >= nbody) return "bodyexclude out of range";
  if (o.exclude_tree && o.bodyexclude < 0) return "exclude_tree needs bodyexclude";
  if (o.align != MJH_HSCAN_ALIGN_YAW && o.align != MJH_HSCAN_ALIGN_BASE && o.align != MJH_HSCAN_ALIGN_WORLD) return "unknown align";
  if (o.width <= 0 || o.height <= 0) return "width and height must be positive";
  if (env0 < 0 || n <= 0 || (long long)env0 + n > nenv) return "env range out of bounds";
  if ((long long)o.width * o.height * n > 0x3fffffffLL) return "n * width * height must stay below 2^30";
  for (int k = 0; k < 2; k++) {
    if (!std::isfinite(o.spacing[k]) || !(o.spacing[k] > 0.0)) return "spacing must be finite and positive";
    if (!std::isfinite(o.offset[k])) return "offset not finite";
    const double half = 0.5 * (double)((k ? o.height : o.width) - 1) * o.spacing[k];
    if (!(std::fabs(o.offset[k]) + half <= HSCAN_FLT_MAX) || !((float)(0.5 * o.spacing[k]) > 0.0f)) return "a cell coordinate overflows";
  }
  if (!std::isfinite(o.above) || !(std::fabs(o.above) <= HSCAN_FLT_MAX)) return "above not finite";
  if (!range) return "null pointer";
  return nullptr;
}

#ifdef __HIPCC__
// The grid frame G (row-major, world = G grid: the columns are gx, gy, gz) of an alignment from the sensor's world rotation S.
//   YAW: gz is the world's z, gx the site's x axis (S's first column) projected onto the world's xy-plane and normalised, gy = gz x gx;
//     a projection of squared length below 1e-6 (the site's x axis within 0.06 degrees of vertical) has no heading: gx is the world's x.
//   BASE: G = S.  WORLD: the identity.
// In YAW and WORLD the third column is exactly (0, 0, 1): the rays go along (0, 0, -1) and the ray parameter is the range.
RDEV void hscan_grid_frame(int align, const float* S, float* G) {
  if (align == MJH_HSCAN_ALIGN_BASE) {
#pragma unroll
    for (int k = 0; k < 9; k++) G[k] = S[k];
    return;
  }
  float gx0 = 1.0f, gx1 = 0.0f;
  if (align == MJH_HSCAN_ALIGN_YAW) {
    const float l2 = S[0]*S[0] + S[3]*S[3];
    if (l2 >= 1e-6f) { const float inv = 1.0f / sqrtf(l2); gx0 = S[0] * inv; gx1 = S[3] * inv; }
  }
  G[0] = gx0; G[1] = -gx1; G[2] = 0.0f;
  G[3] = gx1; G[4] = gx0; G[5] = 0.0f;
  G[6] = 0.0f; G[7] = 0.0f; G[8] = 1.0f;
}

// cell (row i, column j) in the grid frame: x_j = offset_x + (j - (width - 1) / 2) spacing_x = ox + (2 j + 1 - width) hx, y_i likewise.
// The integer factor is exact in fp32 and the product goes into the sum unrounded (fma): one rounding besides those of ox and hx.
RDEV void hscan_cell(int i, int j, int width, int height, float ox, float oy, float hx, float hy, float& x, float& y) {
  x = fmaf((float)(2 * j + 1 - width), hx, ox);
  y = fmaf((float)(2 * i + 1 - height), hy, oy);
}

// the bound of the live cells of a tile, rows [i0, i0 + ni) x columns [j0, j0 + nj): the centre of their extent in the grid frame and
// half its diagonal — every cell of the tile lies within `radius` of (cx, cy)
RDEV void hscan_tile_bound(int i0, int ni, int j0, int nj, int width, int height, float ox, float oy, float hx, float hy, float& cx, float& cy, float& radius) {
  cx = fmaf((float)(2 * j0 + nj - width), hx, ox);
  cy = fmaf((float)(2 * i0 + ni - height), hy, oy);
  const float ex = (float)(nj - 1) * hx, ey = (float)(ni - 1) * hy;
  radius = sqrtf(ex*ex + ey*ey);
}

// Does the sphere (world centre c, radius rb) touch the half-infinite solid cylinder of a tile: axis from the world point a along the
// unit direction u, radius `radius`?  Conservative: true whenever a half-line from a start point on the disc about a, along u, meets
// the sphere.  Such a half-line meets the sphere only if the sphere holds its start (then the centre is at most rb behind the start
// plane) or lies ahead of it, and only if the centre is within rb of the line, which is within `radius` of the axis:
//   h = (c - a) . u >= -rb   and   q = |(c - a) - h u| <= radius + rb.
// The slack covers the fp32 roundings of this test and of the lanes' own origins: both are sums of world coordinates (the sensor's
// origin plus the cell's offset in the grid), each rounding at most 2^-24 = 6e-8 of the magnitudes |a| + radius and |c|, a handful of
// them in a row, and |u| is 1 to a few 1e-7 (a column of a rotation made from a unit quaternion in fp32): 2e-5 of those magnitudes
// is a hundred times that.
RDEV bool hscan_tile_keep(const float* a, const float* u, float radius, const float* c, float rb) {
  const float d[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  const float h = d[0]*u[0] + d[1]*u[1] + d[2]*u[2];
  const float e[3] = {d[0] - h * u[0], d[1] - h * u[1], d[2] - h * u[2]};
  const float q = sqrtf(e[0]*e[0] + e[1]*e[1] + e[2]*e[2]);
  const float mag = fabsf(a[0]) + fabsf(a[1]) + fabsf(a[2]) + fabsf(c[0]) + fabsf(c[1]) + fabsf(c[2]);
  const float slack = 2e-5f * (mag + rb + radius);
  return h >= -(rb + slack) && q <= radius + rb + slack;
}
#endif
