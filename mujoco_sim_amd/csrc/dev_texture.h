// dev_texture.h — 2D textures in the colour image (mjh_render_set_texturing 1): what the texture kernel (texture.hip) adds to dev_ray.h,
// dev_depth.h and dev_render.h — its launch descriptor, a geom's texture record, the hit point in the geom's frame, the half extents the
// mapping divides by and the texel index.  The functions are __host__ __device__: tests/texture_host builds them for the CPU and checks
// the very code the kernel runs.  The mapping is include/mjhip.h's (mjh_render_set_texturing).  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_render.h"

// a geom's texture as the kernel takes it (8 words): tex < 0 for none; adr in texels; width, height >= 1 where tex >= 0
struct TexRec {
  int tex, adr, width, height;
  float rx, ry;                    // texrepeat
  int uniform, pad;
};

struct TextureArgs {
  DepthArgs D;                     // the depth launch's own descriptor: D.depth / D.geomid are read here, never written
  const TexRec* rec;               // [ngeom]
  const unsigned* texels;          // [ntexdata]: one word per texel, R | G << 8 | B << 16 | TEXEL_FLAG
  int ntexdata;
  unsigned* out;                   // [n][height][width]: the texel of a textured hit, TEXEL_NONE elsewhere
};

hipError_t mjh_launch_texture(hipStream_t st, const TextureArgs& A);   // texture.hip

#ifdef __HIPCC__
// the hit point of the world-frame ray (p, v) at parameter x in the frame of a geom (world pose pos, mat), formed as render_normal forms it
RDEV void texture_hit(const float* pos, const float* mat, const float* p, const float* v, float x, float* h) {
  const float d[3] = {p[0] - pos[0], p[1] - pos[1], p[2] - pos[2]};
  const float lp[3] = {mat[0]*d[0] + mat[3]*d[1] + mat[6]*d[2], mat[1]*d[0] + mat[4]*d[1] + mat[7]*d[2], mat[2]*d[0] + mat[5]*d[1] + mat[8]*d[2]};
  const float lv[3] = {mat[0]*v[0] + mat[3]*v[1] + mat[6]*v[2], mat[1]*v[0] + mat[4]*v[1] + mat[7]*v[2], mat[2]*v[0] + mat[5]*v[1] + mat[8]*v[2]};
#pragma unroll
  for (int k = 0; k < 3; k++) h[k] = lp[k] + x * lv[k];
}

// the half extents in x and y the mapping divides by: (1, 1) for a uniform texture, else from the geom's type and its size s in the env
// (a height field: the asset's).  type: RayScene::ginfo's x — a type no texture is defined for (a mesh) takes (1, 1).
RDEV void texture_extent(const RayScene& W, const int4 gi, const float* s, int uniform, float* a) {
  a[0] = a[1] = 1.0f;
  if (uniform) return;
  switch (gi.x) {
    case MJH_GEOM_PLANE: a[0] = s[0] > 0.0f ? s[0] : 1.0f; a[1] = s[1] > 0.0f ? s[1] : 1.0f; break;
    case MJH_GEOM_HFIELD: { const RayHField H = W.hf[gi.w]; a[0] = H.size[0]; a[1] = H.size[1]; } break;
    case MJH_GEOM_SPHERE: case MJH_GEOM_CAPSULE: case MJH_GEOM_CYLINDER: a[0] = a[1] = s[0]; break;
    case MJH_GEOM_ELLIPSOID: case MJH_GEOM_BOX: a[0] = s[0]; a[1] = s[1]; break;
    default: break;
  }
}

// one texture coordinate: the cell of the fractional part of t among n cells.  Always in [0, n - 1]: a coordinate that is not a finite
// number takes cell 0.
RDEV int texture_cell(float t, int n) {
  float f = t - floorf(t);
  if (!(f >= 0.0f && f < 1.0f)) f = 0.0f;
  const int c = (int)floorf(f * (float)n);
  return c < n - 1 ? c : n - 1;
}

// the texel of hit point h (geom frame) under record R and half extents a: its index into the texel table (adr + row * width + column).
// Every operation is rounded on its own (no FMA): the index is defined bit for bit.
RDEV int texture_index(const TexRec& R, const float* a, const float* h) {
#pragma clang fp contract(off)
  const float X = h[0] / a[0], Y = h[1] / a[1];
  const float hx = 0.5f * R.rx, hy = 0.5f * R.ry;
  const float u = hx * X + 0.5f, v = 0.5f - hy * Y;
  return R.adr + texture_cell(v, R.height) * R.width + texture_cell(u, R.width);
}
#endif
