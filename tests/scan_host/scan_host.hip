// scan_host.hip — csrc/dev_scan.h built for the CPU: the pattern checks, the angle tables, the beam directions and the tile cone of the
// scan kernel (with the cone test of dev_depth.h), called by tests/test_scan_host.py through ctypes.
#include "../../mujoco_sim_amd/csrc/dev_scan.h"

extern "C" {

int scan_host_tile_shape(int height) { return scan_tile_shape(height); }

// 0: the pattern is good; 1: it is refused (elevation: [height] or null)
int scan_host_check(int width, int height, long long n, double az0, double az_step, const double* elevation, double el0, double el_step) {
  return scan_pattern_error(width, height, n, az0, az_step, elevation, el0, el_step) ? 1 : 0;
}

// tab [2 (width + height)]
void scan_host_tables(int width, int height, double az0, double az_step, const double* elevation, double el0, double el_step, float* tab) {
  scan_fill_tables(width, height, az0, az_step, elevation, el0, el_step, tab);
}

// out [height][width][3]
void scan_host_dirs(int width, int height, const float* tab, float* out) {
  for (int i = 0; i < height; i++)
    for (int j = 0; j < width; j++) scan_beam_dir(tab, width, height, i, j, out + 3 * ((size_t)i * width + j));
}

// tile (trow, tcol) of every case against its sphere (centre relative to the sensor origin, sensor frame), as the kernel decides:
// keep[k] = 1 unless the tile has a cone and the predicate drops the sphere; cone[k] = the tile has a cone
void scan_host_cull(int width, int height, const float* tab, float az_step, int ncase, const int* trow, const int* tcol, const float* centre,
                    const float* radius, int* keep, int* cone) {
  const int tw_log = scan_tile_shape(height), TW = 1 << tw_log, TH = RAY_TILE >> tw_log;
  for (int k = 0; k < ncase; k++) {
    const int i0 = trow[k] * TH, j0 = tcol[k] * TW;
    const int ni = height - i0 < TH ? height - i0 : TH, nj = width - j0 < TW ? width - j0 : TW;
    float axis[3], cosA, sinA;
    const bool has = scan_tile_cone(tab, width, height, i0, ni, j0, nj, az_step, axis, cosA, sinA);
    cone[k] = has ? 1 : 0;
    keep[k] = (!has || depth_cone_keep(axis, cosA, sinA, centre + 3 * k, radius[k])) ? 1 : 0;
  }
}

}

#ifdef SCAN_HOST_MAIN
// Stand-alone program for the sanitizers (tests/hostbuild.py: sanitized_run): every table, direction and cone of a few patterns —
// partial tiles in both directions, every tile shape — out of heap buffers of exactly the documented sizes, so a read past a table's
// end is reported.  A failure: a beam outside its own tile's cone by more than the predicate's slack.
#include <cstdio>
#include <vector>

int main() {
  struct P { int w, h; double az0, step, el0, elstep; bool table; };
  const P pats[] = {{1, 1, 0.3, 0.0, -0.2, 0.0, false}, {1081, 1, -2.356, 0.004363, 0.0, 0.0, false}, {360, 16, -3.14159, 0.0174533, -0.26, 0.035, false},
                    {3, 5, -0.4, 0.35, -0.5, 0.25, false}, {70, 9, -3.1, 0.0897, 0.0, 0.0, true}, {67, 2, 0.0, -0.05, -1.5, 3.0, false},
                    {33, 3, 1.0, 0.01, -1.5707963267948966, 1.5707963267948966, false}, {3, 4, -3.14159, 2.0944, -0.3, 0.2, false}};
  const double table9[9] = {0.035, -1.396, 0.27, -0.017, 1.396, -0.528, 0.785, 0.0, -0.192};
  int failures = 0; long beams = 0, cones = 0;
  for (const P& p : pats) {
    const double* el = p.table ? table9 : nullptr;
    if (scan_pattern_error(p.w, p.h, 4, p.az0, p.step, el, p.el0, p.elstep)) { failures++; continue; }
    std::vector<float> tab(2 * ((size_t)p.w + p.h));
    scan_fill_tables(p.w, p.h, p.az0, p.step, el, p.el0, p.elstep, tab.data());
    std::vector<float> out(3 * (size_t)p.w * p.h);
    scan_host_dirs(p.w, p.h, tab.data(), out.data());
    const int tw_log = scan_tile_shape(p.h), TW = 1 << tw_log, TH = RAY_TILE >> tw_log;
    for (int i0 = 0; i0 < p.h; i0 += TH)
      for (int j0 = 0; j0 < p.w; j0 += TW) {
        const int ni = p.h - i0 < TH ? p.h - i0 : TH, nj = p.w - j0 < TW ? p.w - j0 : TW;
        float axis[3], cosA, sinA;
        if (!scan_tile_cone(tab.data(), p.w, p.h, i0, ni, j0, nj, (float)std::fabs(p.step), axis, cosA, sinA)) continue;
        cones++;
        for (int i = i0; i < i0 + ni; i++)
          for (int j = j0; j < j0 + nj; j++) {      // a point on every beam, as a sphere of radius 0: the predicate must keep it
            const float* d = out.data() + 3 * ((size_t)i * p.w + j);
            const float c[3] = {2.5f * d[0], 2.5f * d[1], 2.5f * d[2]};
            beams++;
            if (!depth_cone_keep(axis, cosA, sinA, c, 0.0f)) failures++;
          }
      }
  }
  std::printf("scan_host: %ld beams in %ld cones, %d failures\n", beams, cones, failures);
  return failures ? 1 : 0;
}
#endif
