// collide_host.hip — the device's analytic pair routines (csrc/dev_collide.h: __host__ __device__) evaluated on the CPU.
//
// Built two ways by tests/test_collide_host.py, never run on a GPU:
//   * as a shared object: collide_host_pair() / collide_host_batch() run one routine on given geom poses, for the check against the
//     independent fp64 geometry (tests/pairgeom.py);
//   * with -DCOLLIDE_HOST_MAIN and the host part under AddressSanitizer / UBSan as a stand-alone program: every routine on random
//     poses, writing into an exactly-sized heap staging array (a fifth contact would be an out-of-bounds write the sanitizer reports).
// The x86 build does not contract to FMA as the device build does: a rehearsal of the arithmetic and of the control flow.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/mjhip.h"
#include "../../mujoco_sim_amd/csrc/dev_collide.h"

#define COLLIDE_HOST_MAXCON 4      // the largest capacity of an analytic pair (plane - box / cylinder / mesh)

static const float* g_vert = nullptr;
static int g_nvert = 0;

// the vertices (geom frame, [3 * nvert]) plane - mesh pairs use; the caller keeps them alive
extern "C" void collide_host_set_mesh(const float* vert, int nvert) { g_vert = vert; g_nvert = nvert; }

// one pair: positions p[3], rotations m[9] (row-major, world = R local), sizes s[3]; out: up to COLLIDE_HOST_MAXCON records
// {dist, pos[3], normal[3]}.  Returns the number of contacts, -1 for a pair that is not one of the ten analytic ones.
extern "C" int collide_host_pair(int t1, const float* p1, const float* m1, const float* s1, int t2, const float* p2, const float* m2,
                                 const float* s2, float margin, float* out) {
  if (t1 == MJH_GEOM_PLANE) {
    switch (t2) {
      case MJH_GEOM_SPHERE: return c_plane_sphere(p1, m1, p2, s2[0], margin, out, 0);
      case MJH_GEOM_CAPSULE: return c_plane_capsule(p1, m1, p2, m2, s2, margin, out);
      case MJH_GEOM_CYLINDER: return c_plane_cylinder(p1, m1, p2, m2, s2, margin, out);
      case MJH_GEOM_ELLIPSOID: return c_plane_ellipsoid(p1, m1, p2, m2, s2, margin, out);
      case MJH_GEOM_BOX: return c_plane_box(p1, m1, p2, m2, s2, margin, out);
      case MJH_GEOM_MESH: return g_vert ? c_plane_mesh(p1, m1, p2, m2, g_vert, g_nvert, margin, out) : -1;
      default: return -1;
    }
  }
  if (t1 == MJH_GEOM_SPHERE && t2 == MJH_GEOM_SPHERE) return c_sphere_sphere(p1, s1[0], p2, s2[0], margin, out);
  if (t1 == MJH_GEOM_SPHERE && t2 == MJH_GEOM_CAPSULE) return c_sphere_capsule(p1, s1[0], p2, m2, s2, margin, out);
  if (t1 == MJH_GEOM_CAPSULE && t2 == MJH_GEOM_CAPSULE) return c_capsule_capsule(p1, m1, s1, p2, m2, s2, margin, out);
  if (t1 == MJH_GEOM_SPHERE && t2 == MJH_GEOM_BOX) return c_sphere_box(p1, s1[0], p2, m2, s2, margin, out);
  return -1;
}

// n pairs of one type pair: P / M / S are [n][3] / [n][9] / [n][3], out [n][COLLIDE_HOST_MAXCON][7], cnt [n]
extern "C" void collide_host_batch(int n, int t1, const float* P1, const float* M1, const float* S1, int t2, const float* P2, const float* M2,
                                   const float* S2, float margin, float* out, int* cnt) {
  for (int i = 0; i < n; i++)
    cnt[i] = collide_host_pair(t1, P1 + 3 * i, M1 + 9 * i, S1 + 3 * i, t2, P2 + 3 * i, M2 + 9 * i, S2 + 3 * i, margin,
                               out + (size_t)i * COLLIDE_HOST_MAXCON * RAW_STRIDE);
}

#ifdef COLLIDE_HOST_MAIN
namespace {

struct Rng {      // splitmix64: a fixed-seed generator of the program's own
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
};

void pose(Rng& r, float* p, float* m, bool aligned) {
  float q[4] = {r.uni(-1, 1), r.uni(-1, 1), r.uni(-1, 1), r.uni(-1, 1)};
  if (aligned) { q[0] = 1; q[1] = q[2] = q[3] = 0; }
  const float n = std::sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]) + 1e-20f;
  const float w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  m[0] = w*w + x*x - y*y - z*z; m[1] = 2*(x*y - w*z); m[2] = 2*(x*z + w*y);
  m[3] = 2*(x*y + w*z); m[4] = w*w - x*x + y*y - z*z; m[5] = 2*(y*z - w*x);
  m[6] = 2*(x*z - w*y); m[7] = 2*(y*z + w*x); m[8] = w*w - x*x - y*y + z*z;
  for (int k = 0; k < 3; k++) p[k] = r.uni(-0.12f, 0.12f);
}

}  // namespace

int main() {
  Rng r{20261018};
  const int pairs[10][2] = {{MJH_GEOM_PLANE, MJH_GEOM_SPHERE}, {MJH_GEOM_PLANE, MJH_GEOM_CAPSULE}, {MJH_GEOM_PLANE, MJH_GEOM_CYLINDER},
                            {MJH_GEOM_PLANE, MJH_GEOM_ELLIPSOID}, {MJH_GEOM_PLANE, MJH_GEOM_BOX}, {MJH_GEOM_PLANE, MJH_GEOM_MESH},
                            {MJH_GEOM_SPHERE, MJH_GEOM_SPHERE}, {MJH_GEOM_SPHERE, MJH_GEOM_CAPSULE}, {MJH_GEOM_CAPSULE, MJH_GEOM_CAPSULE},
                            {MJH_GEOM_SPHERE, MJH_GEOM_BOX}};
  const int nvert = 13;      // not a multiple of the scan's batch of 8
  float* vert = (float*)std::malloc(sizeof(float) * 3 * nvert);
  for (int i = 0; i < 3 * nvert; i++) vert[i] = r.uni(-0.08f, 0.08f);
  collide_host_set_mesh(vert, nvert);
  long ncon = 0, nbad = 0, ncall = 0;
  for (int it = 0; it < 20000; it++)
    for (int k = 0; k < 10; k++) {
      float p1[3], m1[9], p2[3], m2[9], s1[3], s2[3];
      const bool aligned = it % 4 == 0;      // identical orientations: parallel capsules, standing cylinders, flat boxes
      pose(r, p1, m1, aligned); pose(r, p2, m2, aligned);
      if (it % 16 == 0) for (int q = 0; q < 3; q++) p2[q] = p1[q];      // coincident centres
      for (int q = 0; q < 3; q++) { s1[q] = r.uni(0.03f, 0.12f); s2[q] = r.uni(0.03f, 0.12f); }
      float* out = (float*)std::malloc(sizeof(float) * COLLIDE_HOST_MAXCON * RAW_STRIDE);
      const int n = collide_host_pair(pairs[k][0], p1, m1, s1, pairs[k][1], p2, m2, s2, 0.01f, out);
      ncall++;
      if (n < 0 || n > COLLIDE_HOST_MAXCON) nbad++;
      for (int c = 0; c < n && c < COLLIDE_HOST_MAXCON; c++, ncon++)
        for (int q = 0; q < RAW_STRIDE; q++) if (!std::isfinite(out[c * RAW_STRIDE + q])) { nbad++; break; }
      std::free(out);
    }
  std::free(vert);
  std::printf("collide_host: %ld calls, %ld contacts, %ld failures\n", ncall, ncon, nbad);
  return nbad ? 1 : 0;
}
#endif
