// texture.hip — mjh_texture_kernel: the texel image of a depth / geom-id image pair (mjh_render_set_texturing 1).  A translation unit of
// its own: no instance of the step, ray, depth, shade or light kernels is touched.  mjh_render_device (engine.hip) runs the depth
// launch, then this kernel, then the shade launch (and the light launch) on the same stream: it reads the two images, the exported
// poses, the per-env geom sizes, the geoms' texture records and the texel table, and writes one word per pixel.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_texture.h"

// One workgroup (one wavefront) per (env, tile of DEPTH_TILE x DEPTH_TILE pixels), one pixel per lane: the shade kernel's tiling.  A
// lane regenerates its pixel's ray (RAY_FRAME and depth_pixel_dir, as the depth and shade kernels do), reads its depth and geom id and
// recovers the ray parameter of the hit.  Then the wave serves the distinct winning geoms of the tile one after the other, as the shade
// kernel does: the first pending lane's geom id is made wave-uniform, its pose, size in the env and texture record are wave-uniform
// reads, the lanes that hold that id form their hit point in the geom's frame, compute their texel index and gather one texel each.  A
// geom without a texture retires its lanes with TEXEL_NONE and reads no pose.  No LDS, no barrier.
__global__ __launch_bounds__(RAY_TILE) void mjh_texture_kernel(const TextureArgs A) {
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

  // the pixel: a dead lane of a partial tile, a miss and an id outside the model hold no geom (as in the shade kernel)
  const size_t o = ((size_t)row * (size_t)D.height + (size_t)min(pi, D.height - 1)) * (size_t)D.width + (size_t)min(pj, D.width - 1);
  const float dep = D.depth[o];
  int gid = D.geomid[o];
  if (!live || !(dep >= 0.0f) || gid < 0 || gid >= W.ngeom || !(vv > 0.0f && vv < 3.0e38f)) gid = -1;
  const float x = D.range ? dep / sqrtf(vv) : dep;

  const float* const gsize = W.size + (size_t)env * (size_t)W.size_stride;
  unsigned word = TEXEL_NONE;
  bool pending = gid >= 0;
  for (int round = 0; round < RAY_TILE; round++) {
    const unsigned long long pm = __ballot(pending);
    if (pm == 0) break;
    const int g = __builtin_amdgcn_readlane(gid, (int)__builtin_ctzll(pm));      // (wave-uniform: 0 <= g < ngeom)
    if (pending && gid == g) {
      const TexRec R = A.rec[g];
      if (R.tex >= 0) {
        const int4 gi = W.ginfo[g];
        const float* gp = W.gpos + ((size_t)row * W.ngeom + g) * 3;
        const float* gm = W.gmat + ((size_t)row * W.ngeom + g) * 9;
        float pos[3], mat[9], s[3], a[2], h[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { pos[k] = gp[k]; s[k] = gsize[3*g + k]; }
#pragma unroll
        for (int k = 0; k < 9; k++) mat[k] = gm[k];
        texture_extent(W, gi, s, R.uniform, a);
        texture_hit(pos, mat, p, v, x, h);
        const int idx = texture_index(R, a, h);      // (adr <= idx < adr + width * height by texture_cell)
        word = (idx >= 0 && idx < A.ntexdata) ? A.texels[idx] : TEXEL_NONE;
      }
      pending = false;
    }
  }
  if (!live) return;
  A.out[((size_t)row * (size_t)D.height + (size_t)pi) * (size_t)D.width + (size_t)pj] = word;
}

hipError_t mjh_launch_texture(hipStream_t st, const TextureArgs& A) {
  const DepthArgs& D = A.D;
  if (D.W.n <= 0 || D.width <= 0 || D.height <= 0 || !D.depth || !D.geomid || !A.rec || !A.texels || A.ntexdata <= 0 || !A.out) return hipErrorInvalidValue;
  return ray_launch(mjh_texture_kernel, tile_blocks(D.width, D.height, DEPTH_TILE_LOG, D.W.n), st, A);
}
