// heightscan_host.hip — csrc/dev_heightscan.h built for the CPU: the argument checks, the grid frame, the cell coordinates and the
// cylinder test of the height-scan kernel, called by tests/test_heightscan_host.py through ctypes.
#include "../../mujoco_sim_amd/csrc/dev_heightscan.h"

// the tile (trow, tcol) of a grid as the kernel sees it: the world-frame axis start `a`, the direction `u` and the radius of its cylinder
static void tile_cylinder(int width, int height, const float* o, const float* G, float ox, float oy, float hx, float hy, float above,
                          int trow, int tcol, float* a, float* u, float& radius) {
  const int tw_log = scan_tile_shape(height), TW = 1 << tw_log, TH = RAY_TILE >> tw_log;
  const int i0 = trow * TH, j0 = tcol * TW;
  const int ni = height - i0 < TH ? height - i0 : TH, nj = width - j0 < TW ? width - j0 : TW;
  float cx, cy;
  hscan_tile_bound(i0, ni, j0, nj, width, height, ox, oy, hx, hy, cx, cy, radius);
  for (int k = 0; k < 3; k++) { a[k] = o[k] + G[3*k] * cx + G[3*k+1] * cy + G[3*k+2] * above; u[k] = -G[3*k+2]; }
}

extern "C" {

// 0: the arguments are good; 1: they are refused (range_null: the caller's range pointer is NULL)
int hscan_host_check(int nsite, int nbody, int nenv, int env0, int n, int site, int align, int width, int height, const double* spacing,
                     const double* offset, double above, int bodyexclude, int exclude_tree, int range_null) {
  mjh_heightscan_options o;
  o.site = site; o.align = align; o.width = width; o.height = height; o.spacing[0] = spacing[0]; o.spacing[1] = spacing[1];
  o.offset[0] = offset[0]; o.offset[1] = offset[1]; o.above = above; o.bodyexclude = bodyexclude; o.exclude_tree = exclude_tree;
  o.flg_static = 1; o.cull = 1; o.cutoff = 0.0;
  static float dummy;
  return hscan_args_error(nsite, nbody, nenv, env0, n, o, range_null ? nullptr : &dummy) ? 1 : 0;
}

// G [ncase][9] row-major (columns gx, gy, gz) from S [ncase][9] and the case's alignment
void hscan_host_frames(int ncase, const int* align, const float* S, float* G) {
  for (int k = 0; k < ncase; k++) hscan_grid_frame(align[k], S + 9 * k, G + 9 * k);
}

// x [width], y [height]
void hscan_host_cells(int width, int height, float ox, float oy, float hx, float hy, float* x, float* y) {
  float t;
  for (int j = 0; j < width; j++) hscan_cell(0, j, width, height, ox, oy, hx, hy, x[j], t);
  for (int i = 0; i < height; i++) hscan_cell(i, 0, width, height, ox, oy, hx, hy, t, y[i]);
}

// tile (trow, tcol) of every case against its sphere (world centre, radius), as the kernel decides: o [ncase][3] and G [ncase][9] the
// sensor origin and the grid frame of the case
void hscan_host_cull(int width, int height, float ox, float oy, float hx, float hy, float above, int ncase, const float* o, const float* G,
                     const int* trow, const int* tcol, const float* centre, const float* radius, int* keep) {
  for (int k = 0; k < ncase; k++) {
    float a[3], u[3], r;
    tile_cylinder(width, height, o + 3 * k, G + 9 * k, ox, oy, hx, hy, above, trow[k], tcol[k], a, u, r);
    keep[k] = hscan_tile_keep(a, u, r, centre + 3 * k, radius[k]) ? 1 : 0;
  }
}

}

#ifdef HEIGHTSCAN_HOST_MAIN
// Stand-alone program for the sanitizers (tests/hostbuild.py: sanitized_run): the frames, every cell and every tile's cylinder of a few
// grids — partial tiles in both directions, every tile shape — out of heap buffers of exactly the documented sizes, and the argument
// checks.  A failure: a point on a cell's own ray outside its tile's cylinder, a good call refused or a bad one accepted.
#include <cstdio>
#include <vector>

int main() {
  struct Gd { int w, h; double sx, sy, offx, offy, above; };
  const Gd grids[] = {{41, 23, 0.11, 0.07, 0.0, 0.0, 0.5}, {130, 1, 0.033, 0.1, 0.05, -0.4, 0.5}, {9, 70, 0.45, 0.03, 0.0, 0.0, 0.5},
                      {5, 3, 0.3, 0.25, 0.8, 0.3, 0.5}, {1, 1, 0.1, 0.1, 0.0, 0.0, 0.5}, {64, 64, 0.05, 0.05, -3.0, 7.0, 2.0}};
  // a tilted sensor, and one whose x axis is exactly vertical
  const double qn = std::sqrt(0.98 * 0.98 + 0.05 * 0.05 + 0.08 * 0.08 + 0.15 * 0.15), w = 0.98 / qn, x = 0.05 / qn, y = -0.08 / qn, z = 0.15 / qn;
  const float S_tilt[9] = {(float)(w*w + x*x - y*y - z*z), (float)(2*(x*y - w*z)), (float)(2*(x*z + w*y)), (float)(2*(x*y + w*z)), (float)(w*w - x*x + y*y - z*z),
                           (float)(2*(y*z - w*x)), (float)(2*(x*z - w*y)), (float)(2*(y*z + w*x)), (float)(w*w - x*x - y*y + z*z)};
  const float S_vert[9] = {0.0f, 0.0f, 1.0f, 0.0f, 1.0f, 0.0f, -1.0f, 0.0f, 0.0f};
  const float o[3] = {0.1f, 0.05f, 2.2f};
  int failures = 0; long rays = 0, tiles = 0;
  for (const Gd& g : grids)
    for (int align = 0; align < 3; align++)
      for (const float* S : {S_tilt, S_vert}) {
        mjh_heightscan_options op;
        op.site = -1; op.align = align; op.width = g.w; op.height = g.h; op.spacing[0] = g.sx; op.spacing[1] = g.sy; op.offset[0] = g.offx; op.offset[1] = g.offy;
        op.above = g.above; op.bodyexclude = -1; op.exclude_tree = 0; op.flg_static = 1; op.cull = 1; op.cutoff = 0.0;
        float dummy;
        if (hscan_args_error(1, 2, 4, 0, 4, op, &dummy)) { failures++; continue; }
        float G[9];
        hscan_grid_frame(align, S, G);
        const float ox = (float)g.offx, oy = (float)g.offy, hx = (float)(0.5 * g.sx), hy = (float)(0.5 * g.sy), above = (float)g.above;
        std::vector<float> x((size_t)g.w), y((size_t)g.h);
        hscan_host_cells(g.w, g.h, ox, oy, hx, hy, x.data(), y.data());
        const int tw_log = scan_tile_shape(g.h), TW = 1 << tw_log, TH = RAY_TILE >> tw_log;
        for (int trow = 0; trow * TH < g.h; trow++)
          for (int tcol = 0; tcol * TW < g.w; tcol++) {
            float a[3], u[3], r;
            tile_cylinder(g.w, g.h, o, G, ox, oy, hx, hy, above, trow, tcol, a, u, r);
            tiles++;
            for (int i = trow * TH; i < (trow + 1) * TH && i < g.h; i++)
              for (int j = tcol * TW; j < (tcol + 1) * TW && j < g.w; j++) {      // a point on every ray, as a sphere of radius 0: the predicate must keep it
                float c[3];
                for (int k = 0; k < 3; k++) c[k] = o[k] + G[3*k] * x[j] + G[3*k+1] * y[i] + G[3*k+2] * above + 1.7f * u[k];
                rays++;
                if (!hscan_tile_keep(a, u, r, c, 0.0f)) failures++;
              }
          }
      }
  const double sp[2] = {0.1, 0.1}, off[2] = {0.0, 0.0}, bad_sp[2] = {0.1, 0.0};
  if (hscan_host_check(1, 2, 4, 0, 4, 0, 0, 16, 16, sp, off, 1.0, 1, 1, 0) != 0) failures++;
  if (hscan_host_check(1, 2, 4, 0, 4, 0, 0, 16, 16, bad_sp, off, 1.0, -1, 0, 0) != 1) failures++;
  if (hscan_host_check(1, 2, 4, 0, 4, 0, 0, 16, 16, sp, off, 1.0, -1, 1, 0) != 1) failures++;
  std::printf("heightscan_host: %ld rays in %ld tiles, %d failures\n", rays, tiles, failures);
  return failures ? 1 : 0;
}
#endif
