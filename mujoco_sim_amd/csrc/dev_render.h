// dev_render.h — RGB-D images (mjh_render / mjh_render_device): what the shade kernel (render.hip) adds to dev_ray.h and dev_depth.h — its
// launch descriptor, the surface normal of every geom type a ray can see, resolved on the ONE geom a depth pixel names, and the colour
// of a pixel.  The functions are __host__ __device__: tests/render_host builds them for the CPU and checks the very code the kernel
// runs.  Nothing here walks an env's geoms: the depth launch has done that, the resolve functions take a geom, the ray in the geom's
// frame and the ray parameter x of the hit, so ray.hip can take them later for mjh_ray.  The two table types whose normal needs a
// scan — the height field and a mesh's triangles — have no code here: render_normal calls the NRM instances of dev_ray.h's ray_hfield
// and ray_trimesh, the depth kernel's own walks, so the normal is that of the hit the depth kernel found.  gfx950 only.
//
// A normal is returned in the geom's frame, NOT normalised and NOT oriented (render_finish does both in the world frame).
#pragma once
#include <hip/hip_runtime.h>

#include "dev_depth.h"

struct ShadeArgs {
  DepthArgs D;                     // the depth launch's own descriptor: D.depth / D.geomid are read here, never written
  const float4* color;             // [ngeom] geom_rgba
  float* normal;                   // [n][height][width][3], may be null
  unsigned* rgba;                  // [n][height][width] (R, G, B, A bytes in memory order), may be null
  float ambient, diffuse;
  unsigned background;             // the packed colour of a miss
  const unsigned* texel;           // [n][height][width] the texture kernel's image (dev_texture.h), null without texturing: a pixel's texel
                                   // (R, G, B bytes and TEXEL_FLAG) scales its geom's colour; TEXEL_NONE leaves it as it is
};

#define TEXEL_FLAG 0xff000000u     // the flag byte of a texel word: the pixel's geom carries a texture
#define TEXEL_NONE 0u              // a miss, or a geom without a texture

hipError_t mjh_launch_shade(hipStream_t st, const ShadeArgs& A);   // render.hip

#ifdef __HIPCC__
// ---- the analytic types: the normal at the hit point h (geom frame)
RDEV void normal_ellipsoid(const float* h, const float* s, float* n) {
  n[0] = h[0] / (s[0] * s[0]); n[1] = h[1] / (s[1] * s[1]); n[2] = h[2] / (s[2] * s[2]);
}
RDEV void normal_capsule(const float* h, const float* s, float* n) {
  n[0] = h[0]; n[1] = h[1]; n[2] = h[2] - fminf(fmaxf(h[2], -s[1]), s[1]);
}
// the cap where the point is further outside (or less inside) the cap's plane than the side
RDEV void normal_cylinder(const float* h, const float* s, float* n) {
  const bool cap = fabsf(h[2]) - s[1] >= sqrtf(h[0]*h[0] + h[1]*h[1]) - s[0];
  n[0] = cap ? 0.0f : h[0]; n[1] = cap ? 0.0f : h[1]; n[2] = cap ? (h[2] < 0.0f ? -1.0f : 1.0f) : 0.0f;
}
// the face whose plane the point is nearest to from inside (furthest outside): selects, no indexed array
RDEV void normal_box(const float* h, const float* s, float* n) {
  const float ex = fabsf(h[0]) - s[0], ey = fabsf(h[1]) - s[1], ez = fabsf(h[2]) - s[2];
  const bool fx = ex >= ey && ex >= ez, fy = !fx && ey >= ez;
  n[0] = fx ? (h[0] < 0.0f ? -1.0f : 1.0f) : 0.0f;
  n[1] = fy ? (h[1] < 0.0f ? -1.0f : 1.0f) : 0.0f;
  n[2] = (!fx && !fy) ? (h[2] < 0.0f ? -1.0f : 1.0f) : 0.0f;
}

// ---- the table types
// hull (mesh mode 1): the plane the hit point lies on is the one it is least inside of — the largest n.X - d; the padding planes
// (0, 0, 0, 1) give -1 and a point of the surface about 0 on its own plane.  n and the planes are wave-uniform in the kernel.
RDEV void normal_convex(const float* h, const float4* __restrict__ planes, int num, float* n) {
  float best = -3.0e38f;
  n[0] = n[1] = n[2] = 0.0f;
  for (int k = 0; k < num; k++) {
    const float4 pl = planes[k];
    const float e = pl.x * h[0] + pl.y * h[1] + pl.z * h[2] - pl.w;
    const bool take = e > best;
    best = take ? e : best; n[0] = take ? pl.x : n[0]; n[1] = take ? pl.y : n[1]; n[2] = take ? pl.z : n[2];
  }
}

// triangles (mesh surface 1) and the height field: the feature that gives the hit is only known to the scan that finds it, so the normal
// comes from dev_ray.h's own ray_trimesh<true> / ray_hfield<true> — the one walk the depth kernel took, run again on this geom alone.

// ---- the normal of geom g's surface where the world-frame ray (p, v) meets it at parameter x: the geom's type / table row gi
// (RayScene::ginfo), world pose (pos, mat: row-major, world = mat local) and size s in the env.  nw: world frame, not normalised,
// not oriented; (0, 0, 0) for a type no ray sees.  The ray in the geom's frame is formed as ray_walk forms it.  In the kernel gi, pos,
// mat and s are wave-uniform: the switch is a scalar branch and the table reads are scalar loads.
RDEV void render_normal(const RayScene& W, const RayTris& T, const int4 gi, const float* pos, const float* mat, const float* s,
                        const float* p, const float* v, float x, float* nw) {
  const float d[3] = {p[0] - pos[0], p[1] - pos[1], p[2] - pos[2]};
  const float lp[3] = {mat[0]*d[0] + mat[3]*d[1] + mat[6]*d[2], mat[1]*d[0] + mat[4]*d[1] + mat[7]*d[2], mat[2]*d[0] + mat[5]*d[1] + mat[8]*d[2]};
  const float lv[3] = {mat[0]*v[0] + mat[3]*v[1] + mat[6]*v[2], mat[1]*v[0] + mat[4]*v[1] + mat[7]*v[2], mat[2]*v[0] + mat[5]*v[1] + mat[8]*v[2]};
  const float h[3] = {lp[0] + x * lv[0], lp[1] + x * lv[1], lp[2] + x * lv[2]};
  float n[3] = {0.0f, 0.0f, 0.0f};
  switch (gi.x) {
    case MJH_GEOM_PLANE: n[2] = 1.0f; break;
    case MJH_GEOM_HFIELD: {
      const RayHField H = W.hf[gi.w];
      ray_hfield<true>(lp, lv, H, W.hf_data + H.adr, n);
    } break;
    case MJH_GEOM_SPHERE: n[0] = h[0]; n[1] = h[1]; n[2] = h[2]; break;
    case MJH_GEOM_CAPSULE: normal_capsule(h, s, n); break;
    case MJH_GEOM_ELLIPSOID: normal_ellipsoid(h, s, n); break;
    case MJH_GEOM_CYLINDER: normal_cylinder(h, s, n); break;
    case MJH_GEOM_BOX: normal_box(h, s, n); break;
    case MJH_GEOM_MESH: {
      const RayMesh Mh = W.mesh[gi.w];
      normal_convex(h, W.planes + Mh.adr, Mh.num, n);
    } break;
    case RAY_TYPE_TRIMESH:
      if (T.mesh) {
        const RayTriMesh Mt = T.mesh[gi.w];
        ray_trimesh<true>(lp, lv, Mt, T.nodes + Mt.node, T.tris + (size_t)4 * (size_t)Mt.tri, x + 1e-3f * fabsf(x) + 1e-30f, n);
      }
      break;
    default: break;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) nw[k] = mat[3*k] * n[0] + mat[3*k+1] * n[1] + mat[3*k+2] * n[2];
}

// unit length and orientation towards the ray's origin (n . v <= 0); returns |n . v^| (v^ the unit direction, vv = |v|^2) clamped to
// [0, 1], 1 where it is not a number.  A zero or non-finite normal becomes (0, 0, 0).
RDEV float render_finish(float* n, const float* v, float vv) {
  const float nn = n[0]*n[0] + n[1]*n[1] + n[2]*n[2];
  const bool ok = nn > 0.0f && nn < 3.0e38f;
  const float inv = ok ? 1.0f / sqrtf(nn) : 0.0f;
  const float dot = (n[0]*v[0] + n[1]*v[1] + n[2]*v[2]) * inv;
  const float sg = dot > 0.0f ? -inv : inv;
#pragma unroll
  for (int k = 0; k < 3; k++) n[k] = ok ? n[k] * sg : 0.0f;
  const float c = fabsf(dot) / sqrtf(vv);
  return c <= 1.0f ? c : 1.0f;
}

// a channel: (int)(255 min(1, c) + 0.5) with the product and the sum rounded separately (no FMA: the value is defined bit for bit)
RDEV unsigned render_level(float c) {
#pragma clang fp contract(off)
  const float m = 255.0f * fminf(1.0f, c);
  return (unsigned)(int)(m + 0.5f);
}
RDEV unsigned render_pack(float r, float g, float b, float a) {
  return render_level(r) | (render_level(g) << 8) | (render_level(b) << 16) | (render_level(a) << 24);
}
// the base colour of a textured pixel: the geom's r, g, b times the texel's bytes / 255 (the quotient and the product rounded
// separately), the geom's alpha
RDEV float4 render_texel_base(const float4 col, unsigned t) {
#pragma clang fp contract(off)
  const float tr = (float)(t & 0xffu) / 255.0f, tg = (float)((t >> 8) & 0xffu) / 255.0f, tb = (float)((t >> 16) & 0xffu) / 255.0f;
  return make_float4(col.x * tr, col.y * tg, col.z * tb, col.w);
}
// the colour of a hit: the geom's r, g, b times shade = ambient + diffuse * ndv, alpha 255
RDEV unsigned render_color(const float4 col, float ambient, float diffuse, float ndv) {
#pragma clang fp contract(off)
  const float dl = diffuse * ndv;
  const float shade = ambient + dl;
  return render_level(col.x * shade) | (render_level(col.y * shade) << 8) | (render_level(col.z * shade) << 16) | 0xff000000u;
}
#endif
