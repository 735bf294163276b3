// ray_tri_host.hip — the ray kernels' own triangle walk (csrc/dev_ray.h: ray_tri, ray_trimesh, __host__ __device__) and the BVH builder
// they rely on (csrc/ray_bvh.h, the very file engine.hip includes) evaluated on the CPU.
//
// Built two ways by tests/test_ray_tri_host.py, never run on a GPU:
//   * as a shared object: rth_build() builds the tables of one mesh, the getters hand them out for the invariant checks, and
//     rth_cast() evaluates mesh-frame rays twice — through the BVH (ray_trimesh) and by a loop of the same ray_tri over all triangle
//     records with the same rule of acceptance — for the bit comparison and for the comparison with the fp64 reference;
//   * with -DRAY_TRI_HOST_MAIN and the host part under AddressSanitizer / UBSan as a stand-alone program: tables of meshes of 1 .. 40
//     and of a few thousand triangles in exactly-sized heap arrays, so a read one node or one record past the tables is reported.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mjhip.h"
#include "../../mujoco_sim_amd/csrc/dev_ray.h"

namespace {

// the tables of one mesh in exactly-sized heap arrays
struct Tables {
  RayTriMesh M{}; RayNode* nodes = nullptr; float4* tris = nullptr; RayBvh B;
  bool build(const double* tri, int ntri) {
    clear();
    if (!ray_bvh_build(tri, ntri, B)) return false;
    nodes = (RayNode*)std::malloc(sizeof(RayNode) * B.nodes.size());
    tris = (float4*)std::malloc(sizeof(float) * B.tris.size());
    std::memcpy(nodes, B.nodes.data(), sizeof(RayNode) * B.nodes.size());
    std::memcpy(tris, B.tris.data(), sizeof(float) * B.tris.size());
    M = RayTriMesh{0, (int)B.nodes.size(), 0, ntri, B.rbound, B.r1, 0.0f, 0.0f};
    return true;
  }
  void clear() { std::free(nodes); std::free(tris); nodes = nullptr; tris = nullptr; }
  // the loop of ray_tri over all records, with ray_trimesh's preamble and rule of acceptance
  float brute(const float* p, const float* v, float bound) const {
    const float vn = fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]), pn = fabsf(p[0]) + fabsf(p[1]) + fabsf(p[2]);
    const float L = pn + M.r1, sp = RAY_SLACK * pn;
    float cur = -1.0f, lim = bound;
    for (int t = 0; t < M.ntri; t++) {
      const float x = ray_tri(p, v, vn, L, sp, tris[4*t], tris[4*t + 1], tris[4*t + 2], tris[4*t + 3]);
      if (x >= 0.0f && x <= lim) { cur = x; lim = x; }
    }
    return cur;
  }
  float walk(const float* p, const float* v, float bound) const { return ray_trimesh(p, v, M, nodes, tris, bound); }
};

Tables g_T;

}  // namespace

// -> the node count, or -1
extern "C" int rth_build(const double* tri, int ntri) { return g_T.build(tri, ntri) ? g_T.M.nnode : -1; }
extern "C" void rth_get(float* box /*[n][6]*/, int* skip, int* leaf, int* order /*[ntri]*/, float* rec /*[ntri][16]*/, float* radius /*[2]*/) {
  for (int i = 0; i < g_T.M.nnode; i++) {
    for (int k = 0; k < 3; k++) { box[6*i + k] = g_T.nodes[i].bmin[k]; box[6*i + 3 + k] = g_T.nodes[i].bmax[k]; }
    skip[i] = g_T.nodes[i].skip; leaf[i] = g_T.nodes[i].leaf;
  }
  std::memcpy(order, g_T.B.order.data(), sizeof(int) * g_T.B.order.size());
  std::memcpy(rec, g_T.tris, sizeof(float) * g_T.B.tris.size());
  radius[0] = g_T.M.rbound; radius[1] = g_T.M.r1;
}
// bound[i] < 0: none (3e38, as ray_walk passes it)
extern "C" void rth_cast(int n, const float* P, const float* V, const float* bound, float* bvh, float* brute) {
  for (int i = 0; i < n; i++) {
    const float b = bound && bound[i] >= 0.0f ? bound[i] : 3.0e38f;
    bvh[i] = g_T.walk(P + 3 * i, V + 3 * i, b);
    brute[i] = g_T.brute(P + 3 * i, V + 3 * i, b);
  }
}

#ifdef RAY_TRI_HOST_MAIN
namespace {

struct Rng {      // splitmix64: a fixed-seed generator of the program's own
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  double uni(double lo, double hi) { return lo + (hi - lo) * (double)((next() >> 11) * (1.0 / 9007199254740992.0)); }
};

long g_bad = 0, g_hit = 0, g_ray = 0;

// rays from 3 m and 30 m, from inside, with zero components and along the axes; fresh and with a bound seeded below the fresh hit
void run(Tables& T, Rng& R, long nray) {
  if (!ray_bvh_check(T.B)) g_bad++;
  for (long i = 0; i < nray; i++) {
    float u[3] = {(float)R.uni(-1, 1), (float)R.uni(-1, 1), (float)R.uni(-1, 1)}, t[3], p[3], v[3];
    for (int j = 0; j < 3; j++) t[j] = (float)R.uni(-0.3, 0.3);
    const int fam = (int)(i % 8);
    if (fam >= 5) { u[0] = u[1] = u[2] = 0.0f; u[fam - 5] = (i & 8) ? 1.0f : -1.0f; }
    else if (fam >= 2) u[fam - 2] = 0.0f;
    const float l = std::sqrt(u[0]*u[0] + u[1]*u[1] + u[2]*u[2]) + 1e-20f, back = fam == 1 ? 0.0f : ((i & 1) ? 30.0f : 3.0f), len = (float)R.uni(0.5, 2.0);
    for (int j = 0; j < 3; j++) { p[j] = t[j] + back * u[j] / l; v[j] = -len * u[j] / l; }
    const float a = T.walk(p, v, 3.0e38f), b = T.brute(p, v, 3.0e38f);
    g_ray++; g_hit += a >= 0.0f;
    if (std::memcmp(&a, &b, 4) != 0 || !(a == -1.0f || (a >= 0.0f && std::isfinite(a)))) g_bad++;
    if (a > 0.0f) {      // seeded: a bound just below the hit hides it from both, one at it keeps it
      const float lowb = a * 0.75f, c = T.walk(p, v, lowb), d = T.brute(p, v, lowb), e = T.walk(p, v, a);
      if (std::memcmp(&c, &d, 4) != 0 || c > lowb || e != a) g_bad++;
    }
  }
}

// a torus of nu x nv quads (closed, non-convex), scaled and shifted: 2 nu nv triangles
std::vector<double> torus(int nu, int nv, double R0, double r, double shift) {
  std::vector<double> t;
  auto pt = [&](int i, int j, double* x) { const double a = 6.283185307179586 * (i % nu) / nu, b = 6.283185307179586 * (j % nv) / nv; x[0] = (R0 + r * std::cos(b)) * std::cos(a) + shift; x[1] = (R0 + r * std::cos(b)) * std::sin(a); x[2] = r * std::sin(b) - shift; };
  for (int i = 0; i < nu; i++) for (int j = 0; j < nv; j++) {
    double q[4][3]; pt(i, j, q[0]); pt(i + 1, j, q[1]); pt(i + 1, j + 1, q[2]); pt(i, j + 1, q[3]);
    const int id[6] = {0, 1, 2, 0, 2, 3};
    for (int k : id) t.insert(t.end(), q[k], q[k] + 3);
  }
  return t;
}

}  // namespace

int main() {
  Rng R{77};
  Tables T;
  for (int n = 1; n <= 40; n++) {      // triangle soups of every size that shapes the top of the tree differently
    std::vector<double> t(9 * (size_t)n);
    for (double& x : t) x = R.uni(-0.3, 0.3);
    if (!T.build(t.data(), n)) { g_bad++; continue; }
    run(T, R, 4000);
  }
  { const std::vector<double> t = torus(24, 12, 0.3, 0.1, 0.0); if (T.build(t.data(), (int)t.size() / 9)) run(T, R, 40000); else g_bad++; }
  { const std::vector<double> t = torus(60, 40, 0.25, 0.12, 0.05); if (T.build(t.data(), (int)t.size() / 9)) run(T, R, 20000); else g_bad++; }
  { std::vector<double> t(9, 0.0); if (T.build(t.data(), 1)) run(T, R, 800); else g_bad++; }      // one triangle without area (the model builder drops such; the walk must still be sound)
  { std::vector<double> t(9, 0.0); t[0] = NAN; if (T.build(t.data(), 1)) g_bad++; }               // refused
  T.clear();
  std::printf("%ld rays, %ld hits, %ld failures\n", g_ray, g_hit, g_bad);
  return g_bad ? 1 : 0;
}
#endif
