// texture_host.hip — the texture kernel's own code (csrc/dev_texture.h: __host__ __device__) evaluated on the CPU, behind the depth and
// shade kernels' code as tests/render_host/render_host.hip runs it (included here: depth, geom id and normal come from
// render_host_image).  Built as a shared object by tests/test_texture_host.py, never run on a GPU.  texture_host_image() renders ONE
// env's image from world-frame float32 rays, one pixel per ray, as a lane of mjh_texture_kernel and then of mjh_shade_kernel does: the
// ray parameter recovered from the depth, the geom's record, the half extents, the hit point in the geom's frame, the texel index, one
// gather; then the colour from the texel word (render_texel_base) with the shade kernel's own |n . v^|.
// With -DTEXTURE_HOST_MAIN and the host part under AddressSanitizer / UBSan it is a stand-alone program: random scenes and records over
// exactly-sized heap arrays (an index past a texture is an out-of-bounds read the sanitizer reports), hit points of every size and
// ones that are not numbers.
#include "../render_host/render_host.hip"
#include "../../mujoco_sim_amd/csrc/dev_texture.h"

// rec [ngeom][8]: tex, adr, width, height, rx, ry, uniform, 0 (floats: the integers are small); texels [ntexdata] words as the engine
// packs them.  Outputs beside render_host_image's: word [nray] the texture kernel's image.  rgba is the TEXTURED colour image.
extern "C" int texture_host_image(int ngeom, const float* gpos, const float* gmat, const float* gsize, const int* gtype, const int* gdata,
                                  int nhf, const int* hf_dim, const float* hf_size, const int* hf_adr, const float* hf_data,
                                  int nmesh, const int* plane_adr, const int* plane_num, const float* planes, const float* mesh_rbound,
                                  const int* tri_adr, const int* tri_num, const double* tris, const float* color,
                                  int nray, const float* P, const float* V, int range, float ambient, float diffuse, const float* background,
                                  const float* rec, const unsigned* texels, int ntexdata,
                                  float* depth, int* gid, float* normal, unsigned* rgba, unsigned* word) {
  int rc = render_host_image(ngeom, gpos, gmat, gsize, gtype, gdata, nhf, hf_dim, hf_size, hf_adr, hf_data, nmesh, plane_adr, plane_num, planes,
                             mesh_rbound, tri_adr, tri_num, tris, color, nray, P, V, range, ambient, diffuse, background, depth, gid, normal, rgba);
  if (rc) return rc;
  // what the texture kernel reads of the scene: the geom table and the height fields' sizes
  std::vector<int4> gi((size_t)ngeom);
  for (int g = 0; g < ngeom; g++) gi[g] = make_int4(gtype[g], g + 1, 0, gdata[g]);
  std::vector<RayHField> hf((size_t)(nhf > 0 ? nhf : 1));
  for (int h = 0; h < nhf; h++) {
    hf[h].nrow = hf_dim[2*h]; hf[h].ncol = hf_dim[2*h + 1]; hf[h].adr = hf_adr[h]; hf[h].pad = 0;
    for (int k = 0; k < 4; k++) hf[h].size[k] = hf_size[4*h + k];
  }
  RayScene W{};
  W.ginfo = gi.data(); W.hf = hf.data(); W.hf_data = hf_data; W.ngeom = ngeom;
  for (int i = 0; i < nray; i++) {
    const float* p = P + 3 * i;
    const float* v = V + 3 * i;
    const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
    const int g = gid[i];
    word[i] = TEXEL_NONE;
    if (g < 0 || !(depth[i] >= 0.0f) || !(vv > 0.0f && vv < 3.0e38f)) continue;
    const float* q = rec + 8 * (size_t)g;
    const TexRec R{(int)q[0], (int)q[1], (int)q[2], (int)q[3], q[4], q[5], (int)q[6], 0};
    if (R.tex < 0) continue;
    const float x = range ? depth[i] / sqrtf(vv) : depth[i];
    float a[2], h[3];
    texture_extent(W, gi[g], gsize + 3 * g, R.uniform, a);
    texture_hit(gpos + 3 * g, gmat + 9 * g, p, v, x, h);
    const int idx = texture_index(R, a, h);
    word[i] = (idx >= 0 && idx < ntexdata) ? texels[idx] : TEXEL_NONE;
    if (word[i] & TEXEL_FLAG) {
      // the shade kernel's colour of this lane: its own |n . v^| (the normal before it is normalised), then the textured base colour
      float n[3] = {0.0f, 0.0f, 0.0f};
      RayTris T{nullptr, nullptr, nullptr};
      if (gtype[g] != RAY_TYPE_TRIMESH && gtype[g] != MJH_GEOM_MESH) {
        RayScene Wn = W; Wn.gpos = gpos; Wn.gmat = gmat; Wn.size = gsize;
        render_normal(Wn, T, gi[g], gpos + 3 * g, gmat + 9 * g, gsize + 3 * g, p, v, x, n);
      }
      const float ndv = render_finish(n, v, vv);
      const float4 col = render_texel_base(make_float4(color[4*g], color[4*g+1], color[4*g+2], color[4*g+3]), word[i]);
      rgba[i] = render_color(col, ambient, diffuse, ndv);
    }
  }
  return 0;
}

#ifdef TEXTURE_HOST_MAIN
namespace {

struct TRng {      // splitmix64: a fixed-seed generator of the program's own
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  float uni(float lo, float hi) { return lo + (hi - lo) * (float)((next() >> 40) * (1.0 / 16777216.0)); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

template <class T> T* tight(size_t n) { return (T*)std::malloc(sizeof(T) * (n ? n : 1)); }

long t_bad = 0, t_tex = 0, t_pix = 0;

// the index function alone over hit points of every size, on the seams and not numbers: always inside [adr, adr + width * height)
void run_index(uint64_t seed) {
  TRng R{seed};
  const float special[] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1e-30f, -1e-30f, 1e30f, -1e30f, 3.4e38f, INFINITY, -INFINITY, NAN, 0.99999994f, -0.99999994f};
  const int ns = (int)(sizeof special / sizeof special[0]);
  for (int it = 0; it < 200000; it++) {
    const int w = it % 7 == 0 ? 1 : 1 + R.below(it % 5 == 0 ? 4096 : 9), h = it % 11 == 0 ? 1 : 1 + R.below(it % 3 == 0 ? 4096 : 9);
    const TexRec T{0, R.below(1000), w, h, it % 4 == 0 ? special[R.below(ns)] : R.uni(0.01f, 50.0f), R.uni(0.01f, 50.0f), 0, 0};
    const float a[2] = {it % 9 == 0 ? special[R.below(ns)] : R.uni(0.01f, 3.0f), R.uni(0.01f, 3.0f)};
    float hp[3];
    for (int k = 0; k < 3; k++) hp[k] = it % 2 == 0 ? special[R.below(ns)] : R.uni(-100.0f, 100.0f);
    const int idx = texture_index(T, a, hp);
    t_pix++;
    if (idx < T.adr || idx >= T.adr + w * h) t_bad++;
  }
}

// ngeom geoms of the types a texture is defined for over exactly-sized texel tables; every pixel's word is TEXEL_NONE or an entry of the
// geom's own texture
void run_scene(int ngeom, uint64_t seed, int nray) {
  TRng R{seed};
  const int nhf = 1, ntex = 3;
  const int tw[ntex] = {1, 7, 8}, th[ntex] = {1, 5, 8};
  int tadr[ntex], ntexdata = 0;
  for (int t = 0; t < ntex; t++) { tadr[t] = ntexdata; ntexdata += tw[t] * th[t]; }
  unsigned* texels = tight<unsigned>((size_t)ntexdata);
  for (int t = 0; t < ntex; t++) for (int k = 0; k < tw[t] * th[t]; k++) texels[tadr[t] + k] = TEXEL_FLAG | ((unsigned)t << 16) | (unsigned)k;
  float *gpos = tight<float>(3 * (size_t)ngeom), *gmat = tight<float>(9 * (size_t)ngeom), *size = tight<float>(3 * (size_t)ngeom), *color = tight<float>(4 * (size_t)ngeom);
  float* rec = tight<float>(8 * (size_t)ngeom);
  int *gtype = tight<int>((size_t)ngeom), *gdata = tight<int>((size_t)ngeom);
  int *hf_dim = tight<int>(2), *hf_adr = tight<int>(1);
  float *hf_size = tight<float>(4), *hd = tight<float>(12);
  hf_dim[0] = 3; hf_dim[1] = 4; hf_adr[0] = 0; hf_size[0] = 0.6f; hf_size[1] = 0.4f; hf_size[2] = 0.3f; hf_size[3] = 0.1f;
  for (int k = 0; k < 12; k++) hd[k] = R.uni(0.0f, 1.0f);
  int *plane_adr = tight<int>(0), *plane_num = tight<int>(0), *tri_adr = tight<int>(0), *tri_num = tight<int>(0);
  float *planes = tight<float>(0), *rbound = tight<float>(0);
  double* tris = tight<double>(0);
  for (int g = 0; g < ngeom; g++) {
    const float q[4] = {R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1), R.uni(-1, 1)};
    const float n = std::sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]) + 1e-20f, w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    const float M[9] = {w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x), 2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z};
    for (int k = 0; k < 9; k++) gmat[9 * g + k] = M[k];
    for (int k = 0; k < 3; k++) { gpos[3 * g + k] = R.uni(-2.0f, 2.0f); size[3 * g + k] = g % 13 == 0 ? 0.0f : R.uni(0.1f, 0.4f); }
    for (int k = 0; k < 4; k++) color[4 * g + k] = R.uni(0.0f, 1.0f);
    gtype[g] = g % 7;      // plane .. box
    gdata[g] = gtype[g] == MJH_GEOM_HFIELD ? 0 : -1;
    const int t = g % 4 == 3 ? -1 : R.below(ntex);
    float* r = rec + 8 * (size_t)g;
    r[0] = (float)t; r[1] = (float)(t < 0 ? 0 : tadr[t]); r[2] = (float)(t < 0 ? 1 : tw[t]); r[3] = (float)(t < 0 ? 1 : th[t]);
    r[4] = R.uni(0.05f, 9.0f); r[5] = R.uni(0.05f, 9.0f); r[6] = (float)(g % 2); r[7] = 0.0f;
  }
  float *P = tight<float>(3 * (size_t)nray), *V = tight<float>(3 * (size_t)nray), *depth = tight<float>((size_t)nray), *normal = tight<float>(3 * (size_t)nray);
  int* gid = tight<int>((size_t)nray);
  unsigned *rgba = tight<unsigned>((size_t)nray), *word = tight<unsigned>((size_t)nray);
  for (int i = 0; i < nray; i++) {
    const float t[3] = {R.uni(-2.0f, 2.0f), R.uni(-2.0f, 2.0f), R.uni(-2.0f, 2.0f)};
    for (int k = 0; k < 3; k++) P[3 * i + k] = R.uni(-4.0f, 4.0f);
    const float d[3] = {t[0] - P[3*i], t[1] - P[3*i + 1], t[2] - P[3*i + 2]};
    const float len = R.uni(0.5f, 2.0f) / std::sqrt(d[0]*d[0] + d[1]*d[1] + d[2]*d[2] + 1e-20f);
    for (int k = 0; k < 3; k++) V[3 * i + k] = d[k] * len;
  }
  const float bg[4] = {0.25f, 0.5f, 0.75f, 1.0f};
  for (int range = 0; range < 2; range++) {
    if (texture_host_image(ngeom, gpos, gmat, size, gtype, gdata, nhf, hf_dim, hf_size, hf_adr, hd, 0, plane_adr, plane_num, planes, rbound,
                           tri_adr, tri_num, tris, color, nray, P, V, range, 0.3f, 0.7f, bg, rec, texels, ntexdata, depth, gid, normal, rgba, word) != 0) t_bad++;
    for (int i = 0; i < nray; i++) {
      t_pix++;
      const int g = gid[i];
      const int t = g < 0 ? -1 : (int)rec[8 * (size_t)g];
      if (t < 0) { if (word[i] != TEXEL_NONE) t_bad++; continue; }
      t_tex++;
      const int k = (int)(word[i] & 0xffffu);
      if ((word[i] & TEXEL_FLAG) != TEXEL_FLAG || (int)((word[i] >> 16) & 0xffu) != t || k >= tw[t] * th[t] || (rgba[i] >> 24) != 255u) t_bad++;
    }
  }
  std::free(texels); std::free(gpos); std::free(gmat); std::free(size); std::free(color); std::free(rec); std::free(gtype); std::free(gdata);
  std::free(hf_dim); std::free(hf_adr); std::free(hf_size); std::free(hd); std::free(plane_adr); std::free(plane_num); std::free(tri_adr);
  std::free(tri_num); std::free(planes); std::free(rbound); std::free(tris); std::free(P); std::free(V); std::free(depth); std::free(normal);
  std::free(gid); std::free(rgba); std::free(word);
}

}  // namespace

int main() {
  run_index(77);
  for (int ngeom : {1, 9, 64, 65}) run_scene(ngeom, 266 + (uint64_t)ngeom, 4000);
  std::printf("%ld pixels, %ld textured, %ld failures\n", t_pix, t_tex, t_bad);
  return t_bad ? 1 : 0;
}
#endif
