// render_host.hip — the shade kernel's own code (csrc/dev_render.h: __host__ __device__) evaluated on the CPU, behind the depth kernel's
// own cast (csrc/dev_ray.h: the verdict, the compacted records, the walk).  Built as a shared object by tests/test_render_host.py,
// never run on a GPU: render_host_image() takes one env's scene as plain arrays, builds the tables with the functions the engine builds
// them with (csrc/ray_tables.h: hull planes padded to a multiple of four, a BVH per mesh with triangles) and renders world-frame float32 rays, one pixel per ray,
// as mjh_depth_kernel and mjh_shade_kernel do for a lane: depth and geom id first, then the ray parameter recovered from the depth,
// the normal on the one geom the pixel names, orientation, and the colour.  The comparison with the fp64 reference is tests/render_check.py's.
// With -DRENDER_HOST_MAIN and the host part under AddressSanitizer / UBSan it is a stand-alone program: random scenes of every type over
// exactly-sized heap arrays (a read past a table, an elevation grid or a triangle record is an out-of-bounds read the sanitizer reports),
// every result a unit normal that faces the ray, or a miss.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/mjhip.h"
#include "../../mujoco_sim_amd/csrc/dev_render.h"
#include "../../mujoco_sim_amd/csrc/ray_tables.h"

// gtype: the type a ray sees (MJH_GEOM_*; MJH_GEOM_MESH: the hull of mesh gdata; 8: the triangles of mesh gdata; -1: invisible), gdata:
// hfield / mesh id.  hf_dim [nhf][2] (nrow, ncol), hf_size [nhf][4], hf_adr [nhf] into hf_data.  Per mesh: planes [plane_adr, + plane_num)
// of `planes` (n, d), rbound, triangles [tri_adr, + tri_num) of `tris` (9 doubles each).  color [ngeom][4].  Outputs per ray: depth, gid,
// normal [3], rgba (packed).  Returns 0, or -1 where a BVH could not be built.
extern "C" int render_host_image(int ngeom, const float* gpos, const float* gmat, const float* gsize, const int* gtype, const int* gdata,
                                 int nhf, const int* hf_dim, const float* hf_size, const int* hf_adr, const float* hf_data,
                                 int nmesh, const int* plane_adr, const int* plane_num, const float* planes, const float* mesh_rbound,
                                 const int* tri_adr, const int* tri_num, const double* tris, const float* color,
                                 int nray, const float* P, const float* V, int range, float ambient, float diffuse, const float* background,
                                 float* depth, int* gid, float* normal, unsigned* rgba) {
  std::vector<int4> gi((size_t)ngeom);
  bool any_tri = false;
  for (int g = 0; g < ngeom; g++) { gi[g] = make_int4(gtype[g], g + 1, 0, gdata[g]); any_tri = any_tri || gtype[g] == RAY_TYPE_TRIMESH; }
  std::vector<RayHField> hf((size_t)(nhf > 0 ? nhf : 1));
  for (int h = 0; h < nhf; h++) {
    hf[h].nrow = hf_dim[2*h]; hf[h].ncol = hf_dim[2*h + 1]; hf[h].adr = hf_adr[h]; hf[h].pad = 0;
    for (int k = 0; k < 4; k++) hf[h].size[k] = hf_size[4*h + k];
  }
  std::vector<RayMesh> mesh((size_t)(nmesh > 0 ? nmesh : 1));
  std::vector<float4> pl;
  std::vector<RayTriMesh> tmesh((size_t)(nmesh > 0 ? nmesh : 1), RayTriMesh{0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f});
  std::vector<RayNode> nodes; std::vector<float> trec;
  for (int i = 0; i < nmesh; i++) {
    ray_append_planes(planes + 4 * (size_t)plane_adr[i], plane_num[i], mesh_rbound[i], pl, mesh[i]);
    if (tri_num[i] > 0 && ray_append_bvh(tris + 9 * (size_t)tri_adr[i], tri_num[i], nodes, trec, tmesh[i]) != 0) return -1;
  }
  if (pl.empty()) pl.push_back(make_float4(0.0f, 0.0f, 0.0f, 1.0f));
  if (nodes.empty()) nodes.push_back(RayNode{});
  if (trec.empty()) trec.resize(RAY_TRI_FLOATS, 0.0f);
  RayScene W{};
  W.gpos = gpos; W.gmat = gmat; W.size = gsize; W.size_stride = 0; W.slot_mask = nullptr; W.sbase = 0; W.ginfo = gi.data();
  W.hf = hf.data(); W.hf_data = hf_data; W.mesh = mesh.data(); W.planes = pl.data();
  W.env0 = 0; W.n = 1; W.ngeom = ngeom; W.nbody = ngeom + 1; W.bodyexclude = -1; W.flg_static = 1; W.cutoff = 0.0f;
  RayTris T{nullptr, nullptr, nullptr};
  if (any_tri) { T.mesh = tmesh.data(); T.nodes = nodes.data(); T.tris = (const float4*)trec.data(); }
  const unsigned bg = render_pack(background[0], background[1], background[2], background[3]);

  std::vector<float> recs((size_t)RAY_PASS * RAY_REC);
  for (int i = 0; i < nray; i++) { depth[i] = -1.0f; gid[i] = -1; }
  // the depth kernel's cast: the visible geoms compacted in ascending id, RAY_PASS per pass
  for (int base = 0; base < ngeom; base += RAY_PASS) {
    int cnt = 0;
    for (int lane = 0; lane < RAY_PASS && base + lane < ngeom; lane++) {
      const int g = base + lane;
      float rb;
      const int type = any_tri ? ray_verdict<true>(W, gi[g], gsize + 3 * g, 0u, rb, &T) : ray_verdict<false>(W, gi[g], gsize + 3 * g, 0u, rb);
      if (type < 0) continue;
      ray_store(recs.data() + cnt * RAY_REC, gpos + 3 * g, gmat + 9 * g, gsize + 3 * g, rb, type, gi[g].w, g);
      cnt++;
    }
    for (int i = 0; i < nray; i++) {
      const float* p = P + 3 * i;
      const float* v = V + 3 * i;
      const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
      const bool valid = vv > 0.0f && vv < 3.0e38f;
      if (any_tri) ray_walk<false, true>(W, recs.data(), cnt, p, v, vv, valid, depth[i], gid[i], &T);
      else ray_walk<false, false>(W, recs.data(), cnt, p, v, vv, valid, depth[i], gid[i]);
    }
  }
  // the epilogue of mjh_depth_kernel, then a lane of mjh_shade_kernel
  for (int i = 0; i < nray; i++) {
    const float* p = P + 3 * i;
    const float* v = V + 3 * i;
    const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
    if (range) depth[i] *= sqrtf(vv);
    if (gid[i] < 0) depth[i] = -1.0f;
    float n[3] = {0.0f, 0.0f, 0.0f};
    const int g = gid[i];
    if (g >= 0) {
      const float x = range ? depth[i] / sqrtf(vv) : depth[i];
      render_normal(W, T, gi[g], gpos + 3 * g, gmat + 9 * g, gsize + 3 * g, p, v, x, n);
    }
    const float ndv = render_finish(n, v, vv);
    for (int k = 0; k < 3; k++) normal[3*i + k] = n[k];
    rgba[i] = g >= 0 ? render_color(make_float4(color[4*g], color[4*g+1], color[4*g+2], color[4*g+3]), ambient, diffuse, ndv) : bg;
  }
  return 0;
}

// Both instances of a walk of dev_ray.h on the same geom-frame rays: x0 what the instance without NRM returns, x1 and nrm [nray][3] what
// the one with NRM returns and leaves.  ntri > 0: ray_trimesh over the BVH of `tris` (9 doubles each) with bound[i] per ray; else
// ray_hfield over the nrow x ncol elevations hf_data with hf_size.  Returns 0, or -1 where the BVH could not be built.
extern "C" int render_host_walk_pair(int nrow, int ncol, const float* hf_size, const float* hf_data, int ntri, const double* tris,
                                     int nray, const float* P, const float* V, const float* bound, float* x0, float* x1, float* nrm) {
  if (ntri > 0) {
    std::vector<RayNode> nodes; std::vector<float> trec;
    RayTriMesh M;
    if (ray_append_bvh(tris, ntri, nodes, trec, M) != 0) return -1;
    const float4* q = (const float4*)trec.data();
    for (int i = 0; i < nray; i++) {
      x0[i] = ray_trimesh(P + 3 * i, V + 3 * i, M, nodes.data(), q, bound[i]);
      x1[i] = ray_trimesh<true>(P + 3 * i, V + 3 * i, M, nodes.data(), q, bound[i], nrm + 3 * i);
    }
    return 0;
  }
  RayHField H;
  H.nrow = nrow; H.ncol = ncol; H.adr = 0; H.pad = 0;
  for (int k = 0; k < 4; k++) H.size[k] = hf_size[k];
  for (int i = 0; i < nray; i++) {
    x0[i] = ray_hfield(P + 3 * i, V + 3 * i, H, hf_data);
    x1[i] = ray_hfield<true>(P + 3 * i, V + 3 * i, H, hf_data, nrm + 3 * i);
  }
  return 0;
}

#ifdef RENDER_HOST_MAIN
namespace {

struct Rng {      // splitmix64: a fixed-seed generator of the program's own
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

template <class T> T* exact(size_t n) { return (T*)std::malloc(sizeof(T) * (n ? n : 1)); }

long g_bad = 0, g_hit = 0, g_ray = 0;

// ngeom geoms of every type in turn (plane .. box, hull, triangles, one no ray sees): two height fields of 3 x 4 nodes, two mesh assets,
// each a tetrahedron of four hull planes and (larger, within the same bounding radius) a tetrahedron of four triangles; nray rays from
// around the scene and from inside it
void run_scene(int ngeom, uint64_t seed, int nray) {
  Rng R{seed};
  const int nhf = 2, nmesh = 2;
  float *gpos = exact<float>(3 * (size_t)ngeom), *gmat = exact<float>(9 * (size_t)ngeom), *size = exact<float>(3 * (size_t)ngeom), *color = exact<float>(4 * (size_t)ngeom);
  int *gtype = exact<int>((size_t)ngeom), *gdata = exact<int>((size_t)ngeom);
  int *hf_dim = exact<int>(2 * nhf), *hf_adr = exact<int>(nhf);
  float *hf_size = exact<float>(4 * nhf), *hd = exact<float>(12 * nhf);
  for (int h = 0; h < nhf; h++) {
    hf_dim[2*h] = 3; hf_dim[2*h + 1] = 4; hf_adr[h] = 12 * h;
    hf_size[4*h] = 0.6f; hf_size[4*h + 1] = 0.4f; hf_size[4*h + 2] = 0.3f; hf_size[4*h + 3] = 0.1f;
    for (int k = 0; k < 12; k++) hd[12 * h + k] = R.uni(0.0f, 1.0f);
  }
  int *plane_adr = exact<int>(nmesh), *plane_num = exact<int>(nmesh), *tri_adr = exact<int>(nmesh), *tri_num = exact<int>(nmesh);
  float *planes = exact<float>(16 * nmesh), *rbound = exact<float>(nmesh);
  double* tris = exact<double>(36 * nmesh);
  const float tn[4][3] = {{1, 1, 1}, {1, -1, -1}, {-1, 1, -1}, {-1, -1, 1}};
  for (int m = 0; m < nmesh; m++) {
    // hull: the face planes tn[k] . x / sqrt(3) = d; triangles: the faces of the tetrahedron with the corners -3 d tn[k]
    const float d = 0.1f * (float)(m + 1);
    plane_adr[m] = 4 * m; plane_num[m] = 4; tri_adr[m] = 4 * m; tri_num[m] = 4; rbound[m] = 3.0f * d * 1.7320508f * 1.001f;
    for (int k = 0; k < 4; k++) {
      for (int j = 0; j < 3; j++) planes[16 * m + 4 * k + j] = tn[k][j] * 0.57735027f;
      planes[16 * m + 4 * k + 3] = d;
      int c = 0;
      for (int v = 0; v < 4; v++) if (v != k) { for (int j = 0; j < 3; j++) tris[36 * m + 9 * k + 3 * c + j] = -3.0 * d * 1.7320508 * 0.57735027 * tn[v][j]; c++; }
    }
  }
  for (int g = 0; g < ngeom; g++) {
    const float q[4] = {R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1)};
    const float n = std::sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]) + 1e-20f, w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const float M[9] = {w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x), 2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z};
    for (int k = 0; k < 9; k++) gmat[9 * g + k] = M[k];
    for (int k = 0; k < 3; k++) { gpos[3 * g + k] = R.uni(-2.0f, 2.0f); size[3 * g + k] = R.uni(0.1f, 0.4f); }
    for (int k = 0; k < 4; k++) color[4 * g + k] = R.uni(0.0f, 1.0f);
    const int t = g % 10 == 9 ? -1 : g % 10;      // plane .. mesh hull, triangles (8), then one no ray sees
    gtype[g] = t;
    gdata[g] = t == MJH_GEOM_HFIELD ? R.below(nhf) : (t == MJH_GEOM_MESH || t == RAY_TYPE_TRIMESH) ? R.below(nmesh) : -1;
  }
  float *P = exact<float>(3 * (size_t)nray), *V = exact<float>(3 * (size_t)nray), *depth = exact<float>((size_t)nray), *normal = exact<float>(3 * (size_t)nray);
  int* gid = exact<int>((size_t)nray);
  unsigned* rgba = exact<unsigned>((size_t)nray);
  for (int i = 0; i < nray; i++) {
    const float t[3] = {R.uni(-2.0f, 2.0f), R.uni(-2.0f, 2.0f), R.uni(-2.0f, 2.0f)};
    if (i % 4 == 0) { const int g = R.below(ngeom); for (int k = 0; k < 3; k++) P[3 * i + k] = gpos[3 * g + k] + R.uni(-0.02f, 0.02f); }      // from inside a geom
    else for (int k = 0; k < 3; k++) P[3 * i + k] = R.uni(-4.0f, 4.0f);
    const float d[3] = {t[0] - P[3*i], t[1] - P[3*i + 1], t[2] - P[3*i + 2]};
    const float len = R.uni(0.5f, 2.0f) / std::sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2] + 1e-20f);
    for (int k = 0; k < 3; k++) V[3 * i + k] = d[k] * len;
  }
  const float bg[4] = {0.25f, 0.5f, 0.75f, 1.0f};
  for (int range = 0; range < 2; range++) {
    if (render_host_image(ngeom, gpos, gmat, size, gtype, gdata, nhf, hf_dim, hf_size, hf_adr, hd, nmesh, plane_adr, plane_num, planes, rbound,
                          tri_adr, tri_num, tris, color, nray, P, V, range, 0.3f, 0.7f, bg, depth, gid, normal, rgba) != 0) g_bad++;
    for (int i = 0; i < nray; i++) {
      g_ray++;
      const float* n = normal + 3 * i;
      const float nn = n[0]*n[0] + n[1]*n[1] + n[2]*n[2], nv = n[0]*V[3*i] + n[1]*V[3*i + 1] + n[2]*V[3*i + 2];
      if (gid[i] < -1 || gid[i] >= ngeom || (gid[i] < 0) != (depth[i] == -1.0f)) g_bad++;
      else if (gid[i] < 0) { if (nn != 0.0f || rgba[i] != render_pack(bg[0], bg[1], bg[2], bg[3])) g_bad++; }
      else { g_hit++; if (!(std::fabs(nn - 1.0f) < 1e-5f) || !(nv <= 1e-6f) || (rgba[i] >> 24) != 255u) g_bad++; }
    }
  }
  std::free(gpos); std::free(gmat); std::free(size); std::free(color); std::free(gtype); std::free(gdata); std::free(hf_dim); std::free(hf_adr);
  std::free(hf_size); std::free(hd); std::free(plane_adr); std::free(plane_num); std::free(tri_adr); std::free(tri_num); std::free(planes);
  std::free(rbound); std::free(tris); std::free(P); std::free(V); std::free(depth); std::free(normal); std::free(gid); std::free(rgba);
}

}  // namespace

int main() {
  for (int ngeom : {1, 9, 63, 64, 65, 130}) run_scene(ngeom, 166 + (uint64_t)ngeom, 4000);       // up to, at and past the pass boundary
  std::printf("%ld rays, %ld hits, %ld failures\n", g_ray, g_hit, g_bad);
  return g_bad ? 1 : 0;
}
#endif
