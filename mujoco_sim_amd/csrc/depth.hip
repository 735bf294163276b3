// depth.hip — mjh_depth_kernel: every env's view through a camera of the model, as depth / geom-id images.  A translation unit of its
// own: no instance of the step or ray kernels is touched.  The position-stage launch (PH_FKONLY, engine.hip: mjh_depth_device) has
// exported the envs' geom and body poses; this kernel only reads them, the per-env geom sizes and the slot masks, and writes the
// images.  The rays exist in registers only: generated from the camera's intrinsics and its body's pose in the env.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_depth.h"

// One workgroup (one wavefront) per (env, tile of DEPTH_TILE x DEPTH_TILE pixels), one pixel per lane.  The env's geom records are
// staged RAY_PASS geoms per pass (one per lane) as in ray.hip, but only the visible geoms whose bounding sphere touches the tile's cone
// reach LDS: the survivors are compacted by ballot and a lane prefix count, in ascending geom id (ties break as in ray.hip).  The walk
// then goes over the survivors: the record index is wave-uniform, so the type switch is a scalar branch and the record reads are LDS
// broadcasts.  cull = 0 skips the cone test only: generation and intersection are the same instructions, so the images are the same bits.
static __device__ __forceinline__ float uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

__global__ __launch_bounds__(RAY_TILE) void mjh_depth_kernel(const DepthArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const int lane = (int)threadIdx.x;
  const int tx = (A.width + DEPTH_TILE - 1) / DEPTH_TILE, ty = (A.height + DEPTH_TILE - 1) / DEPTH_TILE, ntile = tx * ty;
  const int row = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - row * ntile;
  if (row >= A.n) return;
  const int env = A.env0 + row;
  const int trow = tile / tx, tcol = tile - trow * tx;
  const int i0 = trow * DEPTH_TILE, j0 = tcol * DEPTH_TILE;
  const int pi = i0 + (lane >> 3), pj = j0 + (lane & 7);
  const bool live = pi < A.height && pj < A.width;

  // the camera's world pose from its body's exported pose, once per env (wave-uniform)
  float p[3], S[9];
  {
    const float* bp = A.xpos + ((size_t)row * A.nbody + A.cam_body) * 3;
    const float* bq = A.xquat + ((size_t)row * A.nbody + A.cam_body) * 4;
    const float w = bq[0], x = bq[1], y = bq[2], z = bq[3];
    const float B[9] = {w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),
                        2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z};
    const float a = A.cam_quat[0], b = A.cam_quat[1], c = A.cam_quat[2], d = A.cam_quat[3];
    const float sw = w*a - x*b - y*c - z*d, sx = w*b + x*a + y*d - z*c, sy = w*c - x*d + y*a + z*b, sz = w*d + x*c - y*b + z*a;
    S[0] = sw*sw + sx*sx - sy*sy - sz*sz; S[1] = 2*(sx*sy - sw*sz); S[2] = 2*(sx*sz + sw*sy);
    S[3] = 2*(sx*sy + sw*sz); S[4] = sw*sw - sx*sx + sy*sy - sz*sz; S[5] = 2*(sy*sz - sw*sx);
    S[6] = 2*(sx*sz - sw*sy); S[7] = 2*(sy*sz + sw*sx); S[8] = sw*sw - sx*sx - sy*sy + sz*sz;
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = bp[k] + B[3*k] * A.cam_pos[0] + B[3*k+1] * A.cam_pos[1] + B[3*k+2] * A.cam_pos[2];
  }
  // the lane's ray (a dead lane of a partial tile casts the ray of the nearest live pixel and stores nothing)
  float dc[3], v[3];
  depth_pixel_dir(min(pi, A.height - 1), min(pj, A.width - 1), A.width, A.height, A.scale, dc);
#pragma unroll
  for (int k = 0; k < 3; k++) v[k] = S[3*k] * dc[0] + S[3*k+1] * dc[1] + S[3*k+2] * dc[2];
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
  const bool valid = vv > 0.0f && vv < 3.0e38f;      // (a non-finite pose sees nothing)
  // the tile's cone in the world frame (wave-uniform): the part of the tile inside the image
  float ac[3], axis[3], cosA, sinA;
  depth_tile_cone(i0, j0, min(DEPTH_TILE, A.height - i0), min(DEPTH_TILE, A.width - j0), A.width, A.height, A.scale, ac, cosA, sinA);
#pragma unroll
  for (int k = 0; k < 3; k++) axis[k] = S[3*k] * ac[0] + S[3*k+1] * ac[1] + S[3*k+2] * ac[2];

  // the camera origin and the cone are wave-uniform: kept in scalar registers
#pragma unroll
  for (int k = 0; k < 3; k++) { p[k] = uniform(p[k]); axis[k] = uniform(axis[k]); }
  cosA = uniform(cosA); sinA = uniform(sinA);

  const unsigned slotmask = A.slot_mask ? A.slot_mask[env] : 0u;
  const float* const gsize = A.size + (size_t)env * (size_t)A.size_stride;

  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < A.ngeom; base += RAY_PASS) {
    __syncthreads();
    const int g = base + lane;
    // stage geom g of this env: the verdict first (type, body, bounding sphere), then only a survivor's record is read and stored
    int4 gi = make_int4(-1, 0, 0, 0);
    float c[3] = {0.0f, 0.0f, 0.0f}, s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, rb = 0.0f;
    bool keep = false;
    if (g < A.ngeom) {
      gi = A.ginfo[g];
      const float* gp = A.gpos + ((size_t)row * A.ngeom + g) * 3;
#pragma unroll
      for (int k = 0; k < 3; k++) c[k] = gp[k];
      s0 = gsize[3*g]; s1 = gsize[3*g + 1]; s2 = gsize[3*g + 2];
      if (gi.x == MJH_GEOM_SPHERE) rb = s0;
      else if (gi.x == MJH_GEOM_CAPSULE) rb = s0 + s1;
      else if (gi.x == MJH_GEOM_ELLIPSOID) rb = fmaxf(s0, fmaxf(s1, s2));
      else if (gi.x == MJH_GEOM_CYLINDER) rb = sqrtf(s0*s0 + s1*s1);
      else if (gi.x == MJH_GEOM_BOX) rb = sqrtf(s0*s0 + s1*s1 + s2*s2);
      else if (gi.x == MJH_GEOM_MESH) rb = A.mesh[gi.w].rbound;
      rb *= 1.001f;     // (as ray.hip: a sphere a little larger than the geom's)
      const bool slot_off = gi.y >= A.sbase && gi.y - A.sbase < 32 && ((slotmask >> (gi.y - A.sbase)) & 1u);
      keep = gi.x >= 0 && gi.y != A.bodyexclude && (A.flg_static || !gi.z) && !slot_off;
      if (keep && A.cull && gi.x >= MJH_GEOM_SPHERE) {      // planes and height fields are never culled
        const float rel[3] = {c[0] - p[0], c[1] - p[1], c[2] - p[2]};
        keep = depth_cone_keep(axis, cosA, sinA, rel, rb);
      }
    }
    const unsigned long long kept = __ballot(keep);
    if (keep) {
      const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
      float* rec = s_rec + slot * RAY_REC;
      const float* gm = A.gmat + ((size_t)row * A.ngeom + g) * 9;
#pragma unroll
      for (int k = 0; k < 3; k++) rec[k] = c[k];
#pragma unroll
      for (int k = 0; k < 9; k++) rec[3 + k] = gm[k];
      rec[12] = s0; rec[13] = s1; rec[14] = s2;
      rec[15] = rb;
      rec[16] = __int_as_float(gi.x);
      rec[17] = __int_as_float(gi.w);
      rec[18] = __int_as_float(g);
      rec[19] = 0.0f;
    }
    __syncthreads();
    const int cnt = __popcll(kept);      // wave-uniform
    for (int j = 0; j < cnt; j++) {
      const float* r = s_rec + j * RAY_REC;
      const int type = __builtin_amdgcn_readfirstlane(__float_as_int(r[16]));
      // the ray in the geom's frame
      const float d[3] = {p[0] - r[0], p[1] - r[1], p[2] - r[2]};
      const float lp[3] = {r[3]*d[0] + r[6]*d[1] + r[9]*d[2], r[4]*d[0] + r[7]*d[1] + r[10]*d[2], r[5]*d[0] + r[8]*d[1] + r[11]*d[2]};
      const float lv[3] = {r[3]*v[0] + r[6]*v[1] + r[9]*v[2], r[4]*v[0] + r[7]*v[1] + r[10]*v[2], r[5]*v[0] + r[8]*v[1] + r[11]*v[2]};
      const float sz[3] = {r[12], r[13], r[14]};
      float x = -1.0f;
      if (type >= MJH_GEOM_SPHERE) {
        // bounding-sphere reject: the origin outside the sphere and the ray pointing away from it, or passing it by
        const float rb = r[15];
        const float b = lp[0]*lv[0] + lp[1]*lv[1] + lp[2]*lv[2], c = lp[0]*lp[0] + lp[1]*lp[1] + lp[2]*lp[2] - rb * rb;
        const float tc = -b / vv;
        const float q[3] = {lp[0] + tc * lv[0], lp[1] + tc * lv[1], lp[2] + tc * lv[2]};
        const bool reject = !valid || (c > 0.0f && (b > 0.0f || q[0]*q[0] + q[1]*q[1] + q[2]*q[2] > rb * rb));
        if (!reject) {
          switch (type) {
            case MJH_GEOM_SPHERE: x = ray_sphere(lp, lv, sz[0]); break;
            case MJH_GEOM_CAPSULE: x = ray_capsule(lp, lv, sz); break;
            case MJH_GEOM_ELLIPSOID: x = ray_ellipsoid(lp, lv, sz); break;
            case MJH_GEOM_CYLINDER: x = ray_cylinder(lp, lv, sz); break;
            case MJH_GEOM_BOX: x = ray_box(lp, lv, sz); break;
            case MJH_GEOM_MESH: {      // the mesh id is wave-uniform: its table row and the planes come by scalar loads
              const int mid = __builtin_amdgcn_readfirstlane(__float_as_int(r[17]));
              const RayMesh Mh = A.mesh[mid];
              x = ray_convex(lp, lv, A.planes + Mh.adr, Mh.num);
            } break;
            default: break;
          }
        }
      } else if (valid) {
        if (type == MJH_GEOM_PLANE) x = ray_plane(lp, lv, sz);
        else {
          const int hid = __builtin_amdgcn_readfirstlane(__float_as_int(r[17]));
          const RayHField H = A.hf[hid];
          x = ray_hfield(lp, lv, H, A.hf_data + H.adr);
        }
      }
      if (x >= 0.0f && (bestg < 0 || x < best)) { best = x; bestg = __float_as_int(r[18]); }
    }
  }
  // dc.z = -1: the ray parameter is the depth along the optical axis; range: the distance from the camera origin
  if (A.range) best *= sqrtf(vv);
  if (A.cutoff > 0.0f && best > A.cutoff) bestg = -1;      // far plane: a value beyond it is a miss
  if (bestg < 0) best = -1.0f;
  if (live) {
    const size_t o = ((size_t)row * (size_t)A.height + (size_t)pi) * (size_t)A.width + (size_t)pj;
    A.depth[o] = best;
    if (A.geomid) A.geomid[o] = bestg;
  }
}

hipError_t mjh_launch_depth(hipStream_t st, const DepthArgs& A) {
  if (A.n <= 0 || A.width <= 0 || A.height <= 0) return hipErrorInvalidValue;
  const long long tx = (A.width + DEPTH_TILE - 1) / DEPTH_TILE, ty = (A.height + DEPTH_TILE - 1) / DEPTH_TILE, blocks = tx * ty * (long long)A.n;
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mjh_depth_kernel, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  return hipGetLastError();
}
