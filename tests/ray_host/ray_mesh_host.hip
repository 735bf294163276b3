// ray_mesh_host.hip — the ray kernel's own half-space clipping (csrc/dev_ray.h: ray_convex, __host__ __device__) evaluated on the CPU.
//
// Built two ways by tests/test_ray_mesh_host.py, never run on a GPU:
//   * as a shared object: ray_mesh_host_cast() evaluates an array of mesh-frame rays against one plane set, for comparison with the
//     fp64 reference (tests/ray_mesh_ref.py: scipy's hull triangles);
//   * with -DRAY_MESH_HOST_MAIN and the host part under AddressSanitizer / UBSan as a stand-alone program: the plane loop over
//     exactly-sized heap arrays of every length 1 .. 13 (the groups of four and the tail) and of 55, 150 and 666 planes, so a read
//     one plane past the set is an out-of-bounds read the sanitizer reports.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/mjhip.h"
#include "../../mujoco_sim_amd/csrc/dev_ray.h"

// dist[i] of ray (P[3i..], V[3i..]) in the frame of the planes (n.x, n.y, n.z, d per plane); the planes are copied into a heap
// array of exactly nplane float4
extern "C" void ray_mesh_host_cast(const float* planes, int nplane, int n, const float* P, const float* V, float* dist) {
  float4* pl = (float4*)std::malloc(sizeof(float4) * (size_t)(nplane > 0 ? nplane : 1));
  if (nplane > 0) std::memcpy(pl, planes, sizeof(float4) * (size_t)nplane);
  for (int i = 0; i < n; i++) dist[i] = ray_convex(P + 3 * i, V + 3 * i, pl, nplane);
  std::free(pl);
}

#ifdef RAY_MESH_HOST_MAIN
namespace {

struct Rng {      // splitmix64: a fixed-seed generator of the program's own
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
};

long g_bad = 0, g_hit = 0, g_ray = 0;

// a result is exactly -1 or a finite distance whose point lies on the solid's surface: inside every plane, on one of them
void tally(const float* pl, int n, const float* p, const float* v, float x) {
  g_ray++;
  if (x == -1.0f) return;
  if (!(x >= 0.0f) || !std::isfinite(x)) { g_bad++; return; }
  g_hit++;
  double worst = -1e30;
  const double len = std::sqrt((double)v[0]*v[0] + (double)v[1]*v[1] + (double)v[2]*v[2]);
  for (int k = 0; k < n; k++) {
    double off = -(double)pl[4*k+3];
    for (int j = 0; j < 3; j++) off += (double)pl[4*k+j] * ((double)p[j] + (double)x * (double)v[j]);
    worst = off > worst ? off : worst;
  }
  const double tol = 1e-5 * (1.0 + (double)x * len);      // (fp32 rounding of a point up to 40 m along the ray)
  if (std::fabs(worst) > tol) g_bad++;
}

// n planes tangent to an ellipsoid with semi-axes (0.3, 0.2, 0.15): a bounded solid from n >= 4 generic normals on (one or two planes
// bound nothing: every result is then -1 or a hit, checked the same way).  The first six normals are the axes: den == 0 exactly
// for rays along an axis.
void run_polytope(int n, uint64_t seed, long nray) {
  Rng R{seed};
  float* pl = (float*)std::malloc(sizeof(float) * 4 * (size_t)n);      // exactly n planes: no slack behind them
  for (int k = 0; k < n; k++) {
    float u[3] = {R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1)};
    if (k < 6) { u[0] = u[1] = u[2] = 0.0f; u[k >> 1] = (k & 1) ? -1.0f : 1.0f; }
    const float l = std::sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]) + 1e-20f;
    for (int j = 0; j < 3; j++) pl[4*k+j] = u[j] / l;
    pl[4*k+3] = std::sqrt(0.09f * pl[4*k]*pl[4*k] + 0.04f * pl[4*k+1]*pl[4*k+1] + 0.0225f * pl[4*k+2]*pl[4*k+2]);
  }
  for (long i = 0; i < nray; i++) {
    const float dist = (i & 1) ? 30.0f : 3.0f;
    float u[3] = {R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1)}, t[3] = {R.uni(-0.1f, 0.1f), R.uni(-0.1f, 0.1f), R.uni(-0.1f, 0.1f)}, p[3], v[3], x;
    const int fam = (int)(i % 8);
    if (fam >= 5) { u[0] = u[1] = u[2] = 0.0f; u[fam - 5] = (i & 8) ? 1.0f : -1.0f; }       // along an axis: parallel to four of the first six planes
    else if (fam >= 2) u[fam - 2] = 0.0f;                                                     // one zero component
    const float l = std::sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]) + 1e-20f;
    const float back = fam == 1 ? 0.0f : dist;                                                // fam 1: the origin inside the solid
    for (int j = 0; j < 3; j++) p[j] = t[j] + back * u[j] / l;
    const float len = R.uni(0.5f, 2.0f);
    for (int j = 0; j < 3; j++) v[j] = -len * u[j] / l;
    if (fam >= 5 && (i & 16) && n >= 6) p[(fam - 4) % 3] = pl[4 * (2 * ((fam - 4) % 3)) + 3];           // ... and exactly in the plane of a face (num == 0)
    float4* q = (float4*)std::malloc(sizeof(float4) * (size_t)n);
    std::memcpy(q, pl, sizeof(float4) * (size_t)n);
    x = ray_convex(p, v, q, n);
    std::free(q);
    tally(pl, n, p, v, x);
  }
  std::free(pl);
}

}  // namespace

int main() {
  for (int n = 1; n <= 13; n++) run_polytope(n, 100 + (uint64_t)n, 20000);
  run_polytope(55, 201, 50000);
  run_polytope(150, 202, 50000);
  run_polytope(666, 203, 20000);
  std::printf("%ld rays, %ld hits, %ld failures\n", g_ray, g_hit, g_bad);
  return g_bad ? 1 : 0;
}
#endif
