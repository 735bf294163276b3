// render.hip — mjh_shade_kernel: world-frame surface normals and a shaded colour image from a depth / geom-id image pair.  A translation
// unit of its own: no instance of the step, ray or depth kernels is touched.  mjh_render_device (engine.hip) runs the depth launch
// exactly as mjh_depth_device issues it and then this kernel on the same stream: it reads the two images, the exported poses, the
// per-env geom sizes and the ray tables, and writes the normal and colour images.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_render.h"

// One workgroup (one wavefront) per (env, tile of DEPTH_TILE x DEPTH_TILE pixels), one pixel per lane: the depth kernel's tiling.  A
// lane regenerates its pixel's ray (RAY_FRAME and depth_pixel_dir, as the depth kernel does), reads its depth and geom id and recovers
// the ray parameter of the hit (the depth itself; depth / |d| under `range`).  Then the wave serves the distinct winning geoms of the
// tile one after the other: while a lane is pending the first pending lane's geom id is made wave-uniform, the lanes that hold that id
// resolve their normals together (render_normal: pose, size, type and table rows by wave-uniform reads, the type switch a scalar
// branch) and leave.  Every round retires at least one lane: at most 64 rounds, one in most tiles.  No LDS, no barrier.
__global__ __launch_bounds__(RAY_TILE) void mjh_shade_kernel(const ShadeArgs A) {
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

  // the pixel: a dead lane of a partial tile, a miss and an id outside the model (a caller's own images) hold no geom
  const size_t o = ((size_t)row * (size_t)D.height + (size_t)min(pi, D.height - 1)) * (size_t)D.width + (size_t)min(pj, D.width - 1);
  const float dep = D.depth[o];
  int gid = D.geomid[o];
  if (!live || !(dep >= 0.0f) || gid < 0 || gid >= W.ngeom || !(vv > 0.0f && vv < 3.0e38f)) gid = -1;
  const float x = D.range ? dep / sqrtf(vv) : dep;

  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;
  float n[3] = {0.0f, 0.0f, 0.0f};
  float4 col = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  bool pending = gid >= 0;
  for (int round = 0; round < RAY_TILE; round++) {
    const unsigned long long pm = __ballot(pending);
    if (pm == 0) break;
    const int g = __builtin_amdgcn_readlane(gid, (int)__builtin_ctzll(pm));      // (wave-uniform: 0 <= g < ngeom)
    if (pending && gid == g) {
      const int4 gi = W.ginfo[g];
      const float* gp = W.gpos + ((size_t)row * W.ngeom + g) * 3;
      const float* gm = W.gmat + ((size_t)row * W.ngeom + g) * 9;
      float pos[3], mat[9], s[3];
#pragma unroll
      for (int k = 0; k < 3; k++) { pos[k] = gp[k]; s[k] = gsize[3*g + k]; }
#pragma unroll
      for (int k = 0; k < 9; k++) mat[k] = gm[k];
      render_normal(W, D.T, gi, pos, mat, s, p, v, x, n);
      col = A.color[g];
      pending = false;
    }
  }
  if (!live) return;
  const float ndv = render_finish(n, v, vv);
  const size_t q = ((size_t)row * (size_t)D.height + (size_t)pi) * (size_t)D.width + (size_t)pj;
  if (A.normal) { A.normal[3*q] = n[0]; A.normal[3*q + 1] = n[1]; A.normal[3*q + 2] = n[2]; }
  if (A.texel && A.rgba && gid >= 0) {      // (texturing 1: the texture kernel's word of this pixel)
    const unsigned t = A.texel[q];
    if (t & TEXEL_FLAG) col = render_texel_base(col, t);
  }
  if (A.rgba) A.rgba[q] = gid >= 0 ? render_color(col, A.ambient, A.diffuse, ndv) : A.background;
}

hipError_t mjh_launch_shade(hipStream_t st, const ShadeArgs& A) {
  const DepthArgs& D = A.D;
  if (D.W.n <= 0 || D.width <= 0 || D.height <= 0 || !D.depth || !D.geomid || !A.color) return hipErrorInvalidValue;
  return ray_launch(mjh_shade_kernel, tile_blocks(D.width, D.height, DEPTH_TILE_LOG, D.W.n), st, A);
}
