// dev_light.h — lights and cast shadows in the colour image (mjh_render_set_lighting 1): what the light kernel (light.hip) adds to
// dev_ray.h, dev_depth.h and dev_render.h — its launch descriptor, the terms of a light at a pixel's hit point, the shadow ray, the
// occluder cull of a tile and the colour.  The functions are __host__ __device__: tests/light_host builds them for the CPU and checks
// the very code the kernel runs.  Nothing of dev_ray.h is changed or instantiated anew: the shadow ray goes through ray_verdict,
// ray_store and ray_walk<false, TRI> exactly as a depth pixel's ray does.  The contract is include/mjhip.h's.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_render.h"

#define LIGHT_DIRECTIONAL 1
#define LIGHT_CASTSHADOW 2

// a light as the kernel takes it (16 words): its frame in its body, colours, cos(cutoff) and the spot exponent
struct LightRec {
  int body, flags;                 // flags: LIGHT_DIRECTIONAL | LIGHT_CASTSHADOW
  float pos[3], dir[3];            // in the body's frame, dir of unit length
  float dif[3], amb[3];
  float coscut, exponent;
};

struct LightArgs {
  DepthArgs D;                     // the depth launch's own descriptor: D.depth / D.geomid are read here, never written
  const float4* color;             // [ngeom] geom_rgba
  const float* normal;             // [n][height][width][3]: the shade launch's normal image, read
  unsigned* rgba;                  // [n][height][width], written
  const unsigned* texel;           // ShadeArgs::texel: null without texturing
  float ambient, diffuse;
  unsigned background;
  int nlight;                      // the ACTIVE lights, in id order
  int shadows, cull;
  float bias;
  LightRec L[MJH_MAXLIGHT];
};

hipError_t mjh_launch_light(hipStream_t st, const LightArgs& A);   // light.hip

#ifdef __HIPCC__
// |n . v^| from the unit normal the normal image holds, clamped as render_finish clamps it (1 where it is not a number)
RDEV float light_ndv(const float* n, const float* v, float vv) {
  const float c = fabsf(n[0]*v[0] + n[1]*v[1] + n[2]*v[2]) / sqrtf(vv);
  return c <= 1.0f ? c : 1.0f;
}

// the light's world position Lw and unit direction dw from its body's exported pose (bp, bq)
RDEV void light_frame(const LightRec& R, const float* bp, const float* bq, float* Lw, float* dw) {
  const float ident[4] = {1.0f, 0.0f, 0.0f, 0.0f};
  float S[9];
  RAY_FRAME(bp, bq, R.pos, ident, Lw, S);
#pragma unroll
  for (int k = 0; k < 3; k++) dw[k] = S[3*k] * R.dir[0] + S[3*k+1] * R.dir[1] + S[3*k+2] * R.dir[2];
}

// the terms of light R (world pose Lw, dw) at the hit point h with unit normal n: returns n . l^ (l^: the unit direction towards the
// light) and leaves spot (1 for a directional light; c^exponent with c = -l^ . d^ inside the cone, 0 outside or where c <= 0).
// A hit point on the light itself (|l| = 0) sees nothing of it.
RDEV float light_terms(const LightRec& R, const float* Lw, const float* dw, const float* h, const float* n, float& spot) {
  if (R.flags & LIGHT_DIRECTIONAL) {
    spot = 1.0f;
    return -(n[0]*dw[0] + n[1]*dw[1] + n[2]*dw[2]);
  }
  const float l[3] = {Lw[0] - h[0], Lw[1] - h[1], Lw[2] - h[2]};
  const float ll = l[0]*l[0] + l[1]*l[1] + l[2]*l[2];
  if (!(ll > 0.0f && ll < 3.0e38f)) { spot = 0.0f; return 0.0f; }
  const float inv = 1.0f / sqrtf(ll);
  const float c = -(l[0]*dw[0] + l[1]*dw[1] + l[2]*dw[2]) * inv;
  spot = (c >= R.coscut && c > 0.0f) ? powf(c, R.exponent) : 0.0f;
  return (n[0]*l[0] + n[1]*l[1] + n[2]*l[2]) * inv;
}

// the shadow ray of a pixel: origin o = h + bias n, direction sv = -d^ (directional: any hit blocks) or L - o (positional: a hit with
// parameter < 1 blocks)
RDEV void light_shadow_ray(const LightRec& R, const float* Lw, const float* dw, const float* h, const float* n, float bias, float* o, float* sv) {
#pragma unroll
  for (int k = 0; k < 3; k++) {
    o[k] = h[k] + bias * n[k];
    sv[k] = (R.flags & LIGHT_DIRECTIONAL) ? -dw[k] : Lw[k] - o[k];
  }
}

// Occluder cull of a tile.  Every shadow origin of the tile lies within rt of ct.  Positional light: the point at parameter s of a
// pixel's segment o -> L is (1 - s) |o - ct| <= rt away from the point at s of the segment ct -> L, so a geom whose bounding sphere
// (centre c, radius rb) is farther than rb + rt from that segment meets no shadow segment of the tile.  Directional light: the rays
// are parallel, the same holds for the ray from ct along -d^.  axis = L - ct (positional) or -d^ (directional).  Conservative: the
// slack covers the fp32 roundings of the distance (a few 1e-7 of the operands' size).
RDEV bool light_cull_keep(const float* ct, float rt, const float* axis, bool directional, const float* c, float rb) {
  const float rel[3] = {c[0] - ct[0], c[1] - ct[1], c[2] - ct[2]};
  const float aa = axis[0]*axis[0] + axis[1]*axis[1] + axis[2]*axis[2];
  float s = aa > 0.0f ? (rel[0]*axis[0] + rel[1]*axis[1] + rel[2]*axis[2]) / aa : 0.0f;
  s = fmaxf(s, 0.0f);
  if (!directional) s = fminf(s, 1.0f);
  const float q[3] = {rel[0] - s * axis[0], rel[1] - s * axis[1], rel[2] - s * axis[2]};
  const float reach = rb + rt;
  const float slack = 2e-5f * (sqrtf(rel[0]*rel[0] + rel[1]*rel[1] + rel[2]*rel[2]) + sqrtf(aa) * s + reach);
  const float lim = reach + slack;
  return !(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] > lim * lim);      // (a distance that is not a number keeps the geom)
}

// the colour of a hit: channel c is level(col[c] * (shade + sum[c])), alpha 255
RDEV unsigned light_color(const float4 col, float shade, const float* sum) {
#pragma clang fp contract(off)
  const float r = shade + sum[0], g = shade + sum[1], b = shade + sum[2];
  return render_level(col.x * r) | (render_level(col.y * g) << 8) | (render_level(col.z * b) << 16) | 0xff000000u;
}
#endif
