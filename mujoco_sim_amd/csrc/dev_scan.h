// dev_scan.h — lidar range images (mjh_scan / mjh_scan_device): what the scan kernel (scan.hip) adds to the scene of dev_ray.h and the
// cone test of dev_depth.h — its launch descriptor, the pattern's checks and angle tables (host), the beam direction and the cone over
// a tile of beams.  The device functions are __host__ __device__: tests/scan_host builds them for the CPU and checks the very code the
// kernel runs.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "dev_depth.h"

#define SCAN_MAXROWS 8   // rows of the tallest tile: a wavefront casts a TH x TW tile of beams, TH TW = RAY_TILE, TH <= SCAN_MAXROWS

struct ScanArgs {
  RayScene W;
  float* range; int* geomid; float* points;   // [n][height][width], [n][height][width], [n][height][width][3]; geomid and points may be null
  const float* tab;                // the pattern's tables (scan_fill_tables): cos az [width], sin az [width], cos el [height], sin el [height]
  int width, height;
  int tw_log;                      // tile shape (scan_tile_shape): TW = 1 << tw_log columns, TH = RAY_TILE >> tw_log rows
  int cull;                        // the tile-cone test
  float az_step;                   // |azimuth_step|: (nj - 1) az_step is the azimuth a tile of nj columns spans
  int site_body; float site_pos[3], site_quat[4];   // sensor frame in its body (site_body < 0: the world frame)
  RayTris T;
};

hipError_t mjh_launch_scan(hipStream_t st, const ScanArgs& A);   // scan.hip

// ---- the pattern on the host (plain C++: the engine and the CPU tests call the same functions)

// log2 of the tile's width: TH is the smallest power of two >= min(height, SCAN_MAXROWS) and TW = RAY_TILE / TH, so a planar scan
// (height 1) casts 1 x 64 tiles with every lane live
inline int scan_tile_shape(int height) {
  int th_log = 0;
  while ((1 << th_log) < (height < SCAN_MAXROWS ? height : SCAN_MAXROWS)) th_log++;
  return 6 - th_log;
}

#define SCAN_HALF_PI 1.5707963267948966
#define SCAN_EL_SLACK 1e-9   // a uniform row at -pi/2 + k (pi / k) may land an ulp of fp64 beyond the pole: such a row is the pole

// the checks of a pattern (elevation: the table [height] or null for elevation0 + i elevation_step): null if it is good, else what is wrong
inline const char* scan_pattern_error(int width, int height, long long n, double azimuth0, double azimuth_step, const double* elevation,
                                      double elevation0, double elevation_step) {
  if (width <= 0 || height <= 0) return "width and height must be positive";
  if (n > 0 && (long long)width * height * n > 0x3fffffffLL) return "n * width * height must stay below 2^30";
  if (!std::isfinite(azimuth0) || !std::isfinite(azimuth_step) || !std::isfinite(azimuth0 + (double)(width - 1) * azimuth_step)) return "azimuth0 / azimuth_step not finite";
  if (elevation) {
    for (int i = 0; i < height; i++)
      if (!std::isfinite(elevation[i]) || std::fabs(elevation[i]) > SCAN_HALF_PI + SCAN_EL_SLACK) return "an elevation table entry is not finite or outside [-pi/2, pi/2]";
  } else {
    if (!std::isfinite(elevation0) || !std::isfinite(elevation_step)) return "elevation0 / elevation_step not finite";
    const double last = elevation0 + (double)(height - 1) * elevation_step;
    if (!std::isfinite(last) || std::fabs(elevation0) > SCAN_HALF_PI + SCAN_EL_SLACK || std::fabs(last) > SCAN_HALF_PI + SCAN_EL_SLACK) return "an elevation row lies outside [-pi/2, pi/2]";
  }
  return nullptr;
}

// the angle tables of a checked pattern, 2 (width + height) floats: cos / sin of every column azimuth and row elevation in fp64, each
// rounded to fp32 once.  cos el is never negative (a row within SCAN_EL_SLACK beyond a pole is the pole): the cone argument needs it.
inline void scan_fill_tables(int width, int height, double azimuth0, double azimuth_step, const double* elevation, double elevation0,
                             double elevation_step, float* tab) {
  for (int j = 0; j < width; j++) {
    const double az = azimuth0 + (double)j * azimuth_step;
    tab[j] = (float)std::cos(az); tab[width + j] = (float)std::sin(az);
  }
  for (int i = 0; i < height; i++) {
    const double el = elevation ? elevation[i] : elevation0 + (double)i * elevation_step;
    const double c = std::cos(el);
    tab[2 * width + i] = (float)(c > 0.0 ? c : 0.0); tab[2 * width + height + i] = (float)std::sin(el);
  }
}

#ifdef __HIPCC__
// beam (row i, column j) in the sensor frame (+x azimuth 0, +z the rotation axis): d = (cos el cos az, cos el sin az, sin el) from the
// two table entries of the row and the two of the column — one product rounding per component besides the tables' own
RDEV void scan_beam_dir(const float* tab, int width, int height, int i, int j, float* d) {
  const float ca = tab[j], sa = tab[width + j], ce = tab[2 * width + i], se = tab[2 * width + height + i];
  d[0] = ce * ca; d[1] = ce * sa; d[2] = se;
}

// The cone over the beams of the tile rows [i0, i0 + ni) x columns [j0, j0 + nj), sensor frame, apex at the origin: false if the tile
// gets no cone (nothing is culled then).  el_lo / el_hi: the lowest and the highest elevation among the tile's own rows (sin el is
// monotonic on [-pi/2, pi/2], so the table need not be ordered).  The axis is the normalised sum of the four extreme beams,
// el_lo / el_hi x first / last column: it lies at the tile's mid azimuth.  cosA is the smallest, sinA the largest (from the cross
// product, as depth_tile_cone) over those four.
//   Why four suffice: with the axis at elevation el_m and a beam D away from it in azimuth, cos theta = sin el sin el_m +
//   cos el cos el_m cos D.  Both cosines of elevations are >= 0, so for a fixed elevation this falls as |D| grows up to pi: the worst
//   column is the first or the last.  For that D, with cos D >= 0, it is a sin el + b cos el with b >= 0 = R cos(el - phi),
//   |phi| <= pi/2, so |el - phi| <= pi, where the cosine has no interior minimum: the worst row is el_lo or el_hi.
// The argument needs the tile's azimuth half-span (nj - 1) az_step / 2 <= pi/2; a tile beyond that (a small width with a large step)
// gets no cone, neither does one whose four beams cancel or whose cone is no narrower than a half-space (cosA <= 0).
RDEV bool scan_tile_cone(const float* tab, int width, int height, int i0, int ni, int j0, int nj, float az_step, float* axis, float& cosA, float& sinA) {
  axis[0] = 0.0f; axis[1] = 0.0f; axis[2] = 1.0f; cosA = -1.0f; sinA = 0.0f;
  if (!((float)(nj - 1) * az_step <= 3.14159f)) return false;
  // (the rows' entries are read once and the extreme rows carried as values, not indices: no load waits for another)
  const float* ce = tab + 2 * width; const float* se = ce + height;
  float ce_lo = ce[i0], se_lo = se[i0], ce_hi = ce_lo, se_hi = se_lo;
  for (int i = i0 + 1; i < i0 + ni; i++) {
    const float c = ce[i], s = se[i];
    if (s < se_lo) { se_lo = s; ce_lo = c; }
    if (s > se_hi) { se_hi = s; ce_hi = c; }
  }
  const float ca[2] = {tab[j0], tab[j0 + nj - 1]}, sa[2] = {tab[width + j0], tab[width + j0 + nj - 1]};
  float b[4][3];      // scan_beam_dir's products
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float c = (k & 2) ? ce_hi : ce_lo;
    b[k][0] = c * ca[k & 1]; b[k][1] = c * sa[k & 1]; b[k][2] = (k & 2) ? se_hi : se_lo;
  }
  const float sx = (b[0][0] + b[1][0]) + (b[2][0] + b[3][0]), sy = (b[0][1] + b[1][1]) + (b[2][1] + b[3][1]), sz = (b[0][2] + b[1][2]) + (b[2][2] + b[3][2]);
  const float ss = sx*sx + sy*sy + sz*sz;
  if (!(ss > 1e-6f)) return false;
  const float inv = 1.0f / sqrtf(ss);
  axis[0] = sx * inv; axis[1] = sy * inv; axis[2] = sz * inv;
  cosA = 1.0f;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float u = b[k][1] * axis[2] - b[k][2] * axis[1], v = b[k][2] * axis[0] - b[k][0] * axis[2], w = b[k][0] * axis[1] - b[k][1] * axis[0];
    cosA = fminf(cosA, b[k][0] * axis[0] + b[k][1] * axis[1] + b[k][2] * axis[2]);
    sinA = fmaxf(sinA, sqrtf(u*u + v*v + w*w));
  }
  return cosA > 0.0f;
}
#endif
