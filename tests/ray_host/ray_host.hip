// ray_host.hip — the ray kernel's own intersection code (csrc/dev_ray.h: __host__ __device__) evaluated on the CPU.
//
// Built two ways by tests/test_ray_host.py, never run on a GPU:
//   * as a shared object: ray_host_cast() evaluates an array of geom-frame rays against one geom, for comparison with the fp64
//     reference (tests/ray_ref.py);
//   * with -DRAY_HOST_MAIN and the host part under AddressSanitizer / UBSan as a stand-alone program: the memory-safety check of the
//     cell walk's row / column clamping.  The elevation lives in an exactly-sized heap array, so a cell index one past the grid is
//     an out-of-bounds read the sanitizer reports.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/mjhip.h"
#include "../../mujoco_sim_amd/csrc/dev_ray.h"

// dist[i] of ray (P[3i..], V[3i..]) in the frame of one geom; hsize / elev (nrow x ncol, row-major) for a height field only
extern "C" void ray_host_cast(int type, const float* size, int nrow, int ncol, const float* hsize, const float* elev, int n, const float* P,
                              const float* V, float* dist) {
  RayHField H{};
  if (type == MJH_GEOM_HFIELD) {
    H.nrow = nrow; H.ncol = ncol; H.adr = 0;
    for (int k = 0; k < 4; k++) H.size[k] = hsize[k];
  }
  for (int i = 0; i < n; i++) {
    const float* p = P + 3 * i;
    const float* v = V + 3 * i;
    float x = -1.0f;
    switch (type) {
      case MJH_GEOM_PLANE: x = ray_plane(p, v, size); break;
      case MJH_GEOM_HFIELD: x = ray_hfield(p, v, H, elev); break;
      case MJH_GEOM_SPHERE: x = ray_sphere(p, v, size[0]); break;
      case MJH_GEOM_CAPSULE: x = ray_capsule(p, v, size); break;
      case MJH_GEOM_ELLIPSOID: x = ray_ellipsoid(p, v, size); break;
      case MJH_GEOM_CYLINDER: x = ray_cylinder(p, v, size); break;
      case MJH_GEOM_BOX: x = ray_box(p, v, size); break;
      default: break;
    }
    dist[i] = x;
  }
}

#ifdef RAY_HOST_MAIN
namespace {

struct Rng {      // splitmix64: a fixed-seed generator of the program's own
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

long g_bad = 0, g_hit = 0, g_ray = 0;

void tally(float x) {
  g_ray++;
  if (x >= 0.0f && std::isfinite(x)) g_hit++;
  else if (x != -1.0f) g_bad++;      // a result is a distance or exactly -1
}

void aim(Rng& R, const float* p, const float* t, float* v) {
  const float d[3] = {t[0] - p[0], t[1] - p[1], t[2] - p[2]};
  const float len = R.uni(0.5f, 2.0f) / std::sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2] + 1e-20f);
  for (int k = 0; k < 3; k++) v[k] = d[k] * len;
}

// the families of tests/ray_ref.py on one terrain: nodes, row / column planes, diagonals, grazing, random (in turn)
void run_terrain(int nrow, int ncol, const float* hsize, uint64_t seed, long nray) {
  Rng R{seed};
  float* elev = (float*)std::malloc(sizeof(float) * (size_t)nrow * (size_t)ncol);      // exactly the grid: no slack behind it
  for (int i = 0; i < nrow * ncol; i++) elev[i] = R.uni(0.0f, 1.0f);
  elev[0] = 0.0f; elev[nrow * ncol - 1] = 1.0f;
  const float sx = hsize[0], sy = hsize[1], sz = hsize[2], sb = hsize[3];
  const float dx = 2.0f * sx / (float)(ncol - 1), dy = 2.0f * sy / (float)(nrow - 1);
  const float zero[3] = {0, 0, 0};
  for (long i = 0; i < nray; i++) {
    float p[3], v[3], t[3], x;
    const int r = R.below(nrow), c = R.below(ncol);      // (border lines and corner nodes included: the clamps are what is checked)
    const float xc = -sx + dx * (float)c, yr = -sy + dy * (float)r;
    switch (i % 6) {
      case 0: p[0] = xc; p[1] = yr; p[2] = sz + R.uni(0.1f, 1.0f); v[0] = v[1] = 0.0f; v[2] = (i & 8) ? 1.0f : -1.0f; if (i & 8) p[2] = -sb - 0.5f; break;
      case 1: p[0] = R.uni(-sx - 1.0f, sx + 1.0f); p[1] = yr; p[2] = R.uni(-sb - 0.5f, sz + 1.5f); t[0] = R.uni(-sx, sx); t[1] = yr; t[2] = R.uni(0.0f, sz);
              aim(R, p, t, v); v[1] = 0.0f; break;
      case 2: p[0] = xc; p[1] = R.uni(-sy - 1.0f, sy + 1.0f); p[2] = R.uni(-sb - 0.5f, sz + 1.5f); t[0] = xc; t[1] = R.uni(-sy, sy); t[2] = R.uni(0.0f, sz);
              aim(R, p, t, v); v[0] = 0.0f; break;
      case 3: { const float k = (float)(1 + R.below(5)) * ((i & 8) ? -1.0f : 1.0f), zc = R.uni(0.15f, 0.6f) * sz;
              p[0] = xc - k * dx; p[1] = yr - k * dy; p[2] = R.uni(0.0f, sz) + std::fabs(k) * zc; v[0] = (k < 0 ? -dx : dx); v[1] = (k < 0 ? -dy : dy); v[2] = -zc; break; }
      case 4: { p[0] = R.uni(-sx, sx); p[1] = R.uni(-sy, sy); p[2] = R.uni(0.0f, sz); const float a = R.uni(0.0f, 6.2831853f), len = R.uni(0.5f, 2.0f);
              v[0] = len * std::cos(a); v[1] = len * std::sin(a); v[2] = len * R.uni(-0.15f, 0.15f); break; }
      default: { const float m = std::fmax(sx, sy) + 1.0f; p[0] = R.uni(-m, m); p[1] = R.uni(-m, m); p[2] = R.uni(-sb - 1.0f, sz + 2.0f);
              t[0] = R.uni(-sx, sx) * 1.05f; t[1] = R.uni(-sy, sy) * 1.05f; t[2] = R.uni(0.0f, sz); aim(R, p, t, v); break; }
    }
    ray_host_cast(MJH_GEOM_HFIELD, zero, nrow, ncol, hsize, elev, 1, p, v, &x);
    tally(x);
  }
  std::free(elev);
}

// every primitive: random rays, one component of vec zeroed, along one axis; origins 3 m and 30 m away
void run_primitives(uint64_t seed, long nray) {
  Rng R{seed};
  const int types[6] = {MJH_GEOM_PLANE, MJH_GEOM_SPHERE, MJH_GEOM_CAPSULE, MJH_GEOM_ELLIPSOID, MJH_GEOM_CYLINDER, MJH_GEOM_BOX};
  const float sizes[6][3] = {{3.0f, 2.0f, 0.05f}, {0.22f, 0, 0}, {0.12f, 0.25f, 0}, {0.3f, 0.18f, 0.12f}, {0.18f, 0.22f, 0}, {0.25f, 0.15f, 0.2f}};
  for (int g = 0; g < 6; g++)
    for (int fam = 0; fam < 7; fam++)
      for (long i = 0; i < nray; i++) {
        const float dist = (i & 1) ? 30.0f : 3.0f;
        float u[3] = {R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1)}, t[3] = {R.uni(-0.3f, 0.3f), R.uni(-0.3f, 0.3f), R.uni(-0.3f, 0.3f)}, p[3], v[3], x;
        if (fam >= 4) { for (int k = 0; k < 3; k++) u[k] = 0.0f; u[fam - 4] = (i & 2) ? 1.0f : -1.0f; }
        else if (fam >= 1) u[fam - 1] = 0.0f;
        const float n = std::sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]) + 1e-20f;
        for (int k = 0; k < 3; k++) p[k] = t[k] + dist * u[k] / n;
        aim(R, p, t, v);
        if (fam >= 4) { for (int k = 0; k < 3; k++) if (k != fam - 4) v[k] = 0.0f; }
        else if (fam >= 1) v[fam - 1] = 0.0f;
        ray_host_cast(types[g], sizes[g], 0, 0, nullptr, nullptr, 1, p, v, &x);
        tally(x);
      }
}

}  // namespace

int main() {
  const float A[4] = {1.5f, 6.0f, 1.0f, 0.1f}, B[4] = {6.0f, 1.5f, 1.0f, 0.1f}, Cs[4] = {4.0f, 2.0f, 0.6f, 0.3f}, D[4] = {1.0f, 0.6f, 0.4f, 0.2f};
  run_terrain(40, 9, A, 61, 200000);
  run_terrain(9, 40, B, 62, 200000);
  run_terrain(17, 33, Cs, 63, 200000);
  run_terrain(2, 2, D, 64, 20000);       // the smallest grid: one cell
  run_primitives(65, 4000);
  std::printf("%ld rays, %ld hits, %ld failures\n", g_ray, g_hit, g_bad);
  return g_bad ? 1 : 0;
}
#endif
