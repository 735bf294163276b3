// light.hip — mjh_light_kernel: the colour image under the model's lights, with cast shadows (mjh_render_set_lighting 1).  A translation
// unit of its own: no instance of the step, ray, depth or shade kernels is touched.  mjh_render_device (engine.hip) runs the depth launch
// and the shade launch (normal only) and then this kernel on the same stream: it reads the depth, geom-id and normal images, the
// exported poses, the per-env geom sizes and the ray tables, and writes the colour image.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_light.h"

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
// rays.  Loop order (decided by measurement; the other one is in history): the env's geoms are staged anew for
// every shadow-casting light, RAY_PASS per pass by ray_stage (dev_ray.h), culled against the tile's shadow segments to THIS light
// (light_cull_keep), and walked by ray_walk.  A lane that needs no ray (a miss, a dead lane of a partial tile, a surface that faces away, a point outside
// the cone, a light that casts no shadow) walks with valid = false and takes nothing; a lane that is blocked stops walking; a pass
// loop is left only when no lane of the wave walks any more (__ballot: wave-uniform, so every barrier is met by the whole wave).
// LDS: the depth kernel's record buffer.  TRI: the instance for scenes with triangle tables, as in depth.hip.
template <bool TRI>
__global__ __launch_bounds__(RAY_TILE) void mjh_light_kernel(const LightArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const DepthArgs& D = A.D;
  const RayScene& W = D.W;
  const int lane = (int)threadIdx.x;
  const int row = tile_row((int)blockIdx.x, D.width, D.height, DEPTH_TILE_LOG);
  if (row >= W.n) return;
  const TileMap tm = tile_map((int)blockIdx.x, row, lane, D.width, D.height, DEPTH_TILE_LOG);
  const int env = W.env0 + row, pi = tm.pi, pj = tm.pj;
  const bool live = tm.live;

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

  const bool cull = A.cull != 0;
  float sum[3] = {0.0f, 0.0f, 0.0f};
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
        const int cnt = ray_stage<TRI>(W, &D.T, s_rec, row, base, lane, slotmask, gsize, [=](bool keep, const int4 gi, const float* c, float rb) {
          if (keep && cull && ray_cullable(gi)) keep = light_cull_keep(ct, rt, axis, directional, c, rb);
          return keep;
        });
        ray_walk<false, TRI>(W, s_rec, cnt, ob, sv, svv, walking, best, bestg, &D.T);
        if (walking && (directional ? bestg >= 0 : best < 1.0f)) { blocked = true; walking = false; }
        if (__ballot(walking) == 0) break;      // (wave-uniform)
      }
    }
    const float t = blocked ? 0.0f : fmaxf(ndl, 0.0f) * spot;
#pragma unroll
    for (int k = 0; k < 3; k++) sum[k] += R.amb[k] + R.dif[k] * t;
  }
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
  return RAY_LAUNCH_TRI(mjh_light_kernel, D.T, tile_blocks(D.width, D.height, DEPTH_TILE_LOG, D.W.n), st, A);
}
