// light.hip — mjh_light_kernel: the colour image under the model's lights, with cast shadows (mjh_render_set_lighting 1).  A translation
// unit of its own: no instance of the step, ray, depth or shade kernels is touched.  mjh_render_device (engine.hip) runs the depth launch
// and the shade launch (normal only) and then this kernel on the same stream: it reads the depth, geom-id and normal images, the
// exported poses, the per-env geom sizes and the ray tables, and writes the colour image.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_light.h"

#ifndef LIGHT_STAGE_ONCE
#define LIGHT_STAGE_ONCE 0   // the loop order of lights against staging passes: 0 restage per light with the cull (the default: it won), 1 stage once per pass
#endif

static __device__ __forceinline__ float uniform(float x) { return ray_float(ray_uniform(ray_bits(x))); }
static __device__ __forceinline__ float wave_min(float x) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) x = fminf(x, __shfl_xor(x, m));
  return x;
}
static __device__ __forceinline__ float wave_max(float x) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) x = fmaxf(x, __shfl_xor(x, m));
  return x;
}

// One workgroup (one wavefront) per (env, tile of DEPTH_TILE x DEPTH_TILE pixels), one pixel per lane: the depth kernel's tiling.  A
// lane regenerates its pixel's ray (RAY_FRAME and depth_pixel_dir, as the depth and shade kernels do), reads its depth, geom id and
// normal and forms the hit point.  Then, light by light (a wave-uniform loop over the records in the kernel arguments): the light's
// world pose from its body's exported pose (scalar), the lane's n . l^ and spot, and — where a lane of the wave needs it — the shadow
// rays.  Loop order: the env's geoms are staged anew for every shadow-casting light, RAY_PASS per pass in ascending geom id by
// ray_verdict / ray_store as the depth kernel stages them, culled against the tile's shadow segments to THIS light (light_cull_keep),
// and walked by ray_walk.  A lane that needs no ray (a miss, a dead lane of a partial tile, a surface that faces away, a point outside
// the cone, a light that casts no shadow) walks with valid = false and takes nothing; a lane that is blocked stops walking; a pass
// loop is left only when no lane of the wave walks any more (__ballot: wave-uniform, so every barrier is met by the whole wave).
// LDS: the depth kernel's record buffer.  TRI: the instance for scenes with triangle tables, as in depth.hip.
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) void mjh_light_kernel(const LightArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const DepthArgs& D = A.D;
  const RayScene& W = D.W;
  const int lane = (int)threadIdx.x;
  const int tx = (D.width + DEPTH_TILE - 1) / DEPTH_TILE, ty = (D.height + DEPTH_TILE - 1) / DEPTH_TILE, ntile = tx * ty;
  const int row = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - row * ntile;
  if (row >= W.n) return;
  const int env = W.env0 + row;
  const int trow = tile / tx, tcol = tile - trow * tx;
  const int pi = trow * DEPTH_TILE + (lane >> 3), pj = tcol * DEPTH_TILE + (lane & 7);
  const bool live = pi < D.height && pj < D.width;

  float p[3], S[9];
  RAY_FRAME(W.xpos + ((size_t)row * W.nbody + D.cam_body) * 3, W.xquat + ((size_t)row * W.nbody + D.cam_body) * 4, D.cam_pos, D.cam_quat, p, S);
  float dc[3], v[3];
  depth_pixel_dir(min(pi, D.height - 1), min(pj, D.width - 1), D.width, D.height, D.scale, dc);
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = S[3*k] * dc[0] + S[3*k+1] * dc[1] + S[3*k+2] * dc[2];
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];

  // the pixel (a dead lane reads the nearest live pixel and holds no geom, as in the shade kernel)
  const size_t o = ((size_t)row * (size_t)D.height + (size_t)min(pi, D.height - 1)) * (size_t)D.width + (size_t)min(pj, D.width - 1);
  const float dep = D.depth[o];
  int gid = D.geomid[o];
  if (!live || !(dep >= 0.0f) || gid < 0 || gid >= W.ngeom || !(vv > 0.0f && vv < 3.0e38f)) gid = -1;
  const bool hit = gid >= 0;
  const float x = D.range ? dep / sqrtf(vv) : dep;
  const float n[3] = {A.normal[3*o], A.normal[3*o + 1], A.normal[3*o + 2]};
  float h[3];
#pragma unroll
  for (int k = 0; k < 3; k++) h[k] = p[k] + x * v[k];

  const unsigned slotmask = W.slot_mask ? W.slot_mask[env] : 0u;
  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;

  float sum[3] = {0.0f, 0.0f, 0.0f};
#if !LIGHT_STAGE_ONCE
  for (int l = 0; l < A.nlight; l++) {
    const LightRec& R = A.L[l];
    const bool directional = (R.flags & LIGHT_DIRECTIONAL) != 0;
    float Lw[3], dw[3];
    light_frame(R, W.xpos + ((size_t)row * W.nbody + R.body) * 3, W.xquat + ((size_t)row * W.nbody + R.body) * 4, Lw, dw);
#pragma unroll
    for (int k = 0; k < 3; k++) { Lw[k] = uniform(Lw[k]); dw[k] = uniform(dw[k]); }
    float spot;
    const float ndl = light_terms(R, Lw, dw, h, n, spot);
    float ob[3], sv[3];
    light_shadow_ray(R, Lw, dw, h, n, A.bias, ob, sv);
    const float svv = sv[0]*sv[0] + sv[1]*sv[1] + sv[2]*sv[2];
    // (a lane without a contribution to lose casts no ray: the result is the same)
    bool walking = hit && A.shadows && (R.flags & LIGHT_CASTSHADOW) && ndl > 0.0f && spot > 0.0f && svv > 0.0f && svv < 3.0e38f;
    bool blocked = false;
    if (__ballot(walking) != 0) {      // (wave-uniform)
      // the sphere around the tile's shadow origins: the centre of their box, the largest distance from it
      float ct[3], rt = 0.0f, axis[3];
#pragma unroll
      for (int k = 0; k < 3; k++) ct[k] = 0.5f * (wave_min(walking ? ob[k] : 3.0e38f) + wave_max(walking ? ob[k] : -3.0e38f));
      {
        const float e[3] = {ob[0] - ct[0], ob[1] - ct[1], ob[2] - ct[2]};
        rt = wave_max(walking ? sqrtf(e[0]*e[0] + e[1]*e[1] + e[2]*e[2]) : 0.0f) * 1.00001f;
      }
#pragma unroll
      for (int k = 0; k < 3; k++) { ct[k] = uniform(ct[k]); axis[k] = directional ? -dw[k] : Lw[k] - ct[k]; }
      rt = uniform(rt);
      // positional: only a hit before the light counts (x < 1: the walk replaces `best` for a strictly smaller x only)
      float best = directional ? -1.0f : 1.0f;
      int bestg = directional ? -1 : W.ngeom;
      for (int base = 0; base < W.ngeom; base += RAY_PASS) {
        __syncthreads();
        const int g = base + lane;
        int4 gi = make_int4(-1, 0, 0, 0);
        float c[3] = {0.0f, 0.0f, 0.0f}, s[3] = {0.0f, 0.0f, 0.0f}, rb = 0.0f;
        bool keep = false;
        if (g < W.ngeom) {
          gi = W.ginfo[g];
          const float* gp = W.gpos + ((size_t)row * W.ngeom + g) * 3;
#pragma unroll
          for (int k = 0; k < 3; k++) c[k] = gp[k];
#pragma unroll
          for (int k = 0; k < 3; k++) s[k] = gsize[3*g + k];
          keep = ray_verdict<TRI>(W, gi, s, slotmask, rb, &D.T) >= 0;
          if (keep && A.cull && gi.x >= MJH_GEOM_SPHERE) keep = light_cull_keep(ct, rt, axis, directional, c, rb);      // planes and height fields are never culled
        }
        const unsigned long long kept = __ballot(keep);
        if (keep) {
          const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
          ray_store(s_rec + slot * RAY_REC, c, W.gmat + ((size_t)row * W.ngeom + g) * 9, s, rb, gi.x, gi.w, g);
        }
        __syncthreads();
        ray_walk<false, TRI>(W, s_rec, __popcll(kept), ob, sv, svv, walking, best, bestg, &D.T);
        if (walking && (directional ? bestg >= 0 : best < 1.0f)) { blocked = true; walking = false; }
        if (__ballot(walking) == 0) break;      // (wave-uniform)
      }
    }
    const float t = blocked ? 0.0f : fmaxf(ndl, 0.0f) * spot;
#pragma unroll
    for (int k = 0; k < 3; k++) sum[k] += R.amb[k] + R.dif[k] * t;
  }
#else
  // The other loop order (an A/B build, -DLIGHT_STAGE_ONCE=1; DESIGN.md section 4d has the numbers): every pass is staged once, without
  // the cull (it is per light), and walked for every light that still has a walking lane.  A lane keeps one bit per light for
  // `walking` and one for `blocked`; the light's frame and the lane's ray are formed again wherever they are needed.  Any hit that
  // counts blocks at once, so no best distance is carried from pass to pass.
  unsigned walkm = 0u, blockm = 0u;
  for (int l = 0; l < A.nlight; l++) {
    const LightRec& R = A.L[l];
    float Lw[3], dw[3], spot, ob[3], sv[3];
    light_frame(R, W.xpos + ((size_t)row * W.nbody + R.body) * 3, W.xquat + ((size_t)row * W.nbody + R.body) * 4, Lw, dw);
    const float ndl = light_terms(R, Lw, dw, h, n, spot);
    light_shadow_ray(R, Lw, dw, h, n, A.bias, ob, sv);
    const float svv = sv[0]*sv[0] + sv[1]*sv[1] + sv[2]*sv[2];
    if (hit && A.shadows && (R.flags & LIGHT_CASTSHADOW) && ndl > 0.0f && spot > 0.0f && svv > 0.0f && svv < 3.0e38f) walkm |= 1u << l;
  }
  if (__ballot(walkm != 0u) != 0) {
    for (int base = 0; base < W.ngeom; base += RAY_PASS) {
      __syncthreads();
      const int g = base + lane;
      int4 gi = make_int4(-1, 0, 0, 0);
      float c[3] = {0.0f, 0.0f, 0.0f}, s[3] = {0.0f, 0.0f, 0.0f}, rb = 0.0f;
      bool keep = false;
      if (g < W.ngeom) {
        gi = W.ginfo[g];
        const float* gp = W.gpos + ((size_t)row * W.ngeom + g) * 3;
#pragma unroll
        for (int k = 0; k < 3; k++) c[k] = gp[k];
#pragma unroll
        for (int k = 0; k < 3; k++) s[k] = gsize[3*g + k];
        keep = ray_verdict<TRI>(W, gi, s, slotmask, rb, &D.T) >= 0;
      }
      const unsigned long long kept = __ballot(keep);
      if (keep) {
        const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
        ray_store(s_rec + slot * RAY_REC, c, W.gmat + ((size_t)row * W.ngeom + g) * 9, s, rb, gi.x, gi.w, g);
      }
      __syncthreads();
      for (int l = 0; l < A.nlight; l++) {
        const bool walking = ((walkm >> l) & 1u) != 0u;
        if (__ballot(walking) == 0) continue;      // (wave-uniform)
        const LightRec& R = A.L[l];
        const bool directional = (R.flags & LIGHT_DIRECTIONAL) != 0;
        float Lw[3], dw[3], ob[3], sv[3];
        light_frame(R, W.xpos + ((size_t)row * W.nbody + R.body) * 3, W.xquat + ((size_t)row * W.nbody + R.body) * 4, Lw, dw);
        light_shadow_ray(R, Lw, dw, h, n, A.bias, ob, sv);
        const float svv = sv[0]*sv[0] + sv[1]*sv[1] + sv[2]*sv[2];
        float best = directional ? -1.0f : 1.0f;
        int bestg = directional ? -1 : W.ngeom;
        ray_walk<false, TRI>(W, s_rec, __popcll(kept), ob, sv, svv, walking, best, bestg, &D.T);
        if (walking && (directional ? bestg >= 0 : best < 1.0f)) { blockm |= 1u << l; walkm &= ~(1u << l); }
      }
      if (__ballot(walkm != 0u) == 0) break;      // (wave-uniform)
    }
  }
  for (int l = 0; l < A.nlight; l++) {
    const LightRec& R = A.L[l];
    float Lw[3], dw[3], spot;
    light_frame(R, W.xpos + ((size_t)row * W.nbody + R.body) * 3, W.xquat + ((size_t)row * W.nbody + R.body) * 4, Lw, dw);
    const float ndl = light_terms(R, Lw, dw, h, n, spot);
    const float t = ((blockm >> l) & 1u) ? 0.0f : fmaxf(ndl, 0.0f) * spot;
#pragma unroll
    for (int k = 0; k < 3; k++) sum[k] += R.amb[k] + R.dif[k] * t;
  }
#endif
  if (!live) return;
  const size_t q = ((size_t)row * (size_t)D.height + (size_t)pi) * (size_t)D.width + (size_t)pj;
  unsigned out = A.background;
  if (hit) {
    const float shade = A.ambient + A.diffuse * light_ndv(n, v, vv);
    float4 col = A.color[gid];
    if (A.texel) {      // (texturing 1: the texture kernel's word of this pixel)
      const unsigned t = A.texel[q];
      if (t & TEXEL_FLAG) col = render_texel_base(col, t);
    }
    out = light_color(col, shade, sum);
  }
  A.rgba[q] = out;
}

hipError_t mjh_launch_light(hipStream_t st, const LightArgs& A) {
  const DepthArgs& D = A.D;
  if (D.W.n <= 0 || D.width <= 0 || D.height <= 0 || !D.depth || !D.geomid || !A.color || !A.normal || !A.rgba) return hipErrorInvalidValue;
  if (A.nlight < 0 || A.nlight > MJH_MAXLIGHT || !D.W.xpos || !D.W.xquat) return hipErrorInvalidValue;
  for (int l = 0; l < A.nlight; l++) if (A.L[l].body < 0 || A.L[l].body >= D.W.nbody) return hipErrorInvalidValue;
  const long long tx = (D.width + DEPTH_TILE - 1) / DEPTH_TILE, ty = (D.height + DEPTH_TILE - 1) / DEPTH_TILE, blocks = tx * ty * (long long)D.W.n;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  if (D.T.mesh) hipLaunchKernelGGL(mjh_light_kernel<true>, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  else hipLaunchKernelGGL(mjh_light_kernel<false>, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  return hipGetLastError();
}
