// ray_host.hip — the ray and depth kernels' own code (csrc/dev_ray.h: __host__ __device__) evaluated on the CPU: the intersections,
// and the frame composition, verdict, record and walk that take a ray through an env's geoms.
//
// Built two ways by tests/test_ray_host.py, never run on a GPU:
//   * as a shared object: ray_host_cast() evaluates an array of geom-frame rays against one geom and ray_host_scene() world-frame
//     rays against a whole scene, for comparison with the fp64 references (tests/ray_ref.py, tests/ray_mesh_ref.py);
//   * with -DRAY_HOST_MAIN and the host part under AddressSanitizer / UBSan as a stand-alone program: the memory-safety check of the
//     cell walk's row / column clamping and of the scene cast.  The elevation, the staged records, ginfo and every table live in
//     exactly-sized heap arrays, so a cell index one past the grid or a read past a record or a table is an out-of-bounds read
//     the sanitizer reports.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
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

// World-frame rays through a whole scene of one env with the kernels' shared code (dev_ray.h: ray_verdict, ray_store, ray_walk): the
// geoms are staged in passes of RAY_PASS, one record per geom as ray.hip does (an invisible geom's record has type -1 and the walk
// skips it), or with `compact` only the visible geoms, in ascending id from record 0, as depth.hip does (its walk has no skip).  W.n is
// 1: gpos / gmat are the env's; W.env0 selects the env's row of slot_mask and size.  dist / geomid [nray] as the kernels report them.
extern "C" void ray_host_scene(const RayScene* Wp, int compact, int nray, const float* P, const float* V, float* dist, int* geomid) {
  const RayScene& W = *Wp;
  const unsigned slotmask = W.slot_mask ? W.slot_mask[W.env0] : 0u;
  const float* const gsize = W.size + (size_t)W.env0 * (size_t)W.size_stride;
  float* const recs = (float*)std::malloc(sizeof(float) * RAY_PASS * RAY_REC);      // exactly one pass: no slack behind it
  for (int i = 0; i < nray; i++) { dist[i] = -1.0f; geomid[i] = -1; }
  for (int base = 0; base < W.ngeom; base += RAY_PASS) {
    int cnt = 0;
    for (int lane = 0; lane < RAY_PASS && base + lane < W.ngeom; lane++) {
      const int g = base + lane;
      const int4 gi = W.ginfo[g];
      float rb;
      const int type = ray_verdict(W, gi, gsize + 3 * g, slotmask, rb);
      if (compact && type < 0) continue;
      ray_store(recs + (compact ? cnt : lane) * RAY_REC, W.gpos + 3 * g, W.gmat + 9 * g, gsize + 3 * g, rb, type, gi.w, g);
      cnt = compact ? cnt + 1 : lane + 1;
    }
    for (int i = 0; i < nray; i++) {
      const float* p = P + 3 * i;
      const float* v = V + 3 * i;
      const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
      const bool valid = vv > 0.0f && vv < 3.0e38f;
      if (compact) ray_walk<false>(W, recs, cnt, p, v, vv, valid, dist[i], geomid[i]);
      else ray_walk<true>(W, recs, cnt, p, v, vv, valid, dist[i], geomid[i]);
    }
  }
  for (int i = 0; i < nray; i++) {
    if (W.cutoff > 0.0f && dist[i] > W.cutoff) geomid[i] = -1;
    if (geomid[i] < 0) dist[i] = -1.0f;
  }
  std::free(recs);
}

// n frames given in bodies: body poses bp [n][3], bq [n][4], frames pos [n][3], quat [n][4] -> world origins o [n][3], rotations S [n][9]
extern "C" void ray_host_frame(int n, const float* bp, const float* bq, const float* pos, const float* quat, float* o, float* S) {
  for (int i = 0; i < n; i++) RAY_FRAME(bp + 3 * i, bq + 4 * i, pos + 3 * i, quat + 4 * i, o + 3 * i, S + 9 * i);
}
// the layout of RayScene for the test's ctypes mirror: the offset of every field in declaration order, then the size
extern "C" void ray_host_scene_layout(int* out) {
  const size_t off[] = {offsetof(RayScene, gpos), offsetof(RayScene, gmat), offsetof(RayScene, xpos), offsetof(RayScene, xquat), offsetof(RayScene, size),
                        offsetof(RayScene, size_stride), offsetof(RayScene, slot_mask), offsetof(RayScene, sbase), offsetof(RayScene, ginfo), offsetof(RayScene, hf),
                        offsetof(RayScene, hf_data), offsetof(RayScene, mesh), offsetof(RayScene, planes), offsetof(RayScene, env0), offsetof(RayScene, n),
                        offsetof(RayScene, ngeom), offsetof(RayScene, nbody), offsetof(RayScene, bodyexclude), offsetof(RayScene, flg_static),
                        offsetof(RayScene, cutoff), sizeof(RayScene)};
  for (size_t k = 0; k < sizeof(off) / sizeof(off[0]); k++) out[k] = (int)off[k];
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

// the scene cast over heap arrays sized exactly to the scene: ngeom geoms of every type (nhf height fields of 3 x 4 nodes, nmesh
// tetrahedra of 4 planes), some on an excluded body, some static, some in an inactive slot, some with a ginfo type of -1
template <class T> T* exact(size_t n) { return (T*)std::malloc(sizeof(T) * (n ? n : 1)); }

void run_scene(int ngeom, uint64_t seed, int nray) {
  Rng R{seed};
  const int nhf = 2, nmesh = 2, nbody = 40;
  float *gpos = exact<float>(3 * (size_t)ngeom), *gmat = exact<float>(9 * (size_t)ngeom), *size = exact<float>(3 * (size_t)ngeom);
  int4* gi = exact<int4>((size_t)ngeom);
  unsigned* mask = exact<unsigned>(1);
  RayHField* hf = exact<RayHField>(nhf);
  float* hd = exact<float>(12 * nhf);
  RayMesh* mesh = exact<RayMesh>(nmesh);
  float4* planes = exact<float4>(4 * nmesh);
  for (int h = 0; h < nhf; h++) {
    hf[h].nrow = 3; hf[h].ncol = 4; hf[h].adr = 12 * h; hf[h].pad = 0;
    hf[h].size[0] = 0.6f; hf[h].size[1] = 0.4f; hf[h].size[2] = 0.3f; hf[h].size[3] = 0.1f;
    for (int k = 0; k < 12; k++) hd[12 * h + k] = R.uni(0.0f, 1.0f);
  }
  const float tn[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
  for (int m = 0; m < nmesh; m++) {
    mesh[m].adr = 4 * m; mesh[m].num = 4; mesh[m].rbound = 0.3f * (float)(m + 1); mesh[m].pad = 0.0f;
    for (int k = 0; k < 4; k++) planes[4 * m + k] = make_float4(tn[k][0] * 0.57735027f, tn[k][1] * 0.57735027f, tn[k][2] * 0.57735027f, 0.1f * (float)(m + 1));
  }
  mask[0] = 0x00010004u;      // bodies sbase + 2 and sbase + 16 are inactive
  for (int g = 0; g < ngeom; g++) {
    const float q[4] = {R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1)};
    const float n = std::sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]) + 1e-20f, w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const float M[9] = {w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x), 2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z};
    for (int k = 0; k < 9; k++) gmat[9 * g + k] = M[k];
    for (int k = 0; k < 3; k++) { gpos[3 * g + k] = R.uni(-2.0f, 2.0f); size[3 * g + k] = R.uni(0.1f, 0.4f); }
    const int t = g % 9 == 8 ? -1 : g % 9;      // plane .. mesh in turn, then one no ray sees
    gi[g] = make_int4(t, R.below(nbody), R.below(4) == 0, t == MJH_GEOM_HFIELD ? R.below(nhf) : t == MJH_GEOM_MESH ? R.below(nmesh) : -1);
  }
  float *P = exact<float>(3 * (size_t)nray), *V = exact<float>(3 * (size_t)nray), *dist = exact<float>((size_t)nray);
  int* gid = exact<int>((size_t)nray);
  for (int i = 0; i < nray; i++) {
    const float t[3] = {R.uni(-2.0f, 2.0f), R.uni(-2.0f, 2.0f), R.uni(-2.0f, 2.0f)};
    for (int k = 0; k < 3; k++) P[3 * i + k] = R.uni(-4.0f, 4.0f);
    aim(R, P + 3 * i, t, V + 3 * i);
  }
  RayScene W{};
  W.gpos = gpos; W.gmat = gmat; W.size = size; W.size_stride = 0; W.slot_mask = mask; W.sbase = nbody - 32; W.ginfo = gi;
  W.hf = hf; W.hf_data = hd; W.mesh = mesh; W.planes = planes; W.env0 = 0; W.n = 1; W.ngeom = ngeom; W.nbody = nbody;
  for (int mode = 0; mode < 4; mode++) {
    W.bodyexclude = (mode & 1) ? 3 : -1; W.flg_static = (mode & 2) ? 0 : 1;
    for (int compact = 0; compact < 2; compact++) {
      ray_host_scene(&W, compact, nray, P, V, dist, gid);
      for (int i = 0; i < nray; i++) {
        tally(dist[i]);
        if (gid[i] < -1 || gid[i] >= ngeom || (gid[i] < 0) != (dist[i] == -1.0f)) g_bad++;
      }
    }
  }
  std::free(gpos); std::free(gmat); std::free(size); std::free(gi); std::free(mask); std::free(hf); std::free(hd); std::free(mesh); std::free(planes);
  std::free(P); std::free(V); std::free(dist); std::free(gid);
}

}  // namespace

int main() {
  const float A[4] = {1.5f, 6.0f, 1.0f, 0.1f}, B[4] = {6.0f, 1.5f, 1.0f, 0.1f}, Cs[4] = {4.0f, 2.0f, 0.6f, 0.3f}, D[4] = {1.0f, 0.6f, 0.4f, 0.2f};
  run_terrain(40, 9, A, 61, 200000);
  run_terrain(9, 40, B, 62, 200000);
  run_terrain(17, 33, Cs, 63, 200000);
  run_terrain(2, 2, D, 64, 20000);       // the smallest grid: one cell
  run_primitives(65, 4000);
  for (int ngeom : {1, 63, 64, 65, 130}) run_scene(ngeom, 66 + (uint64_t)ngeom, 2000);       // up to, at and past the pass boundary; a last partial pass
  std::printf("%ld rays, %ld hits, %ld failures\n", g_ray, g_hit, g_bad);
  return g_bad ? 1 : 0;
}
#endif
