// ray.hip — mjh_ray_kernel: batched ray casting against the geoms of every environment (mj_ray semantics; the laser scans and
// range finders the reference's robots carry).  A translation unit of its own: no instance of the step kernels is touched.
// The position-stage launch (PH_FKONLY, engine.hip: mjh_ray_device) has exported the envs' geom (and body) poses; this kernel only
// reads them, the per-env geom sizes and the slot masks, and writes dist / geomid.  gfx950 only.
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "dev_ray.h"

// One workgroup (one wavefront) per (env, tile of RAY_TILE rays), one ray per lane.  The env's geom records are staged into LDS,
// RAY_PASS geoms per pass (one per lane); then every lane walks the records together: the geom index is wave-uniform, so the type
// switch is a scalar branch and the record reads are LDS broadcasts.  Envs are addressed by env id (env0 + row of the launch).
__global__ __launch_bounds__(RAY_TILE) void mjh_ray_kernel(const RayArgs A) {
  __shared__ float s_rec[RAY_PASS * RAY_REC];
  const int lane = (int)threadIdx.x;
  const int ntile = (A.nray + RAY_TILE - 1) / RAY_TILE;
  const int row = (int)blockIdx.x / ntile, tile = (int)blockIdx.x - row * ntile;
  if (row >= A.n) return;
  const int env = A.env0 + row;
  const int ray = tile * RAY_TILE + lane;
  const bool live = ray < A.nray;
  const size_t ro = ((A.per_env ? (size_t)row * (size_t)A.nray : 0) + (size_t)min(ray, A.nray - 1)) * 3;
  float p[3] = {A.pnt[ro], A.pnt[ro + 1], A.pnt[ro + 2]}, v[3] = {A.vec[ro], A.vec[ro + 1], A.vec[ro + 2]};

  if (A.site_body >= 0) {      // site frame -> world: the site's pose from its body's exported pose, once per env (wave-uniform)
    const float* bp = A.xpos + ((size_t)row * A.nbody + A.site_body) * 3;
    const float* bq = A.xquat + ((size_t)row * A.nbody + A.site_body) * 4;
    const float w = bq[0], x = bq[1], y = bq[2], z = bq[3];
    const float B[9] = {w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),
                        2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z};
    const float a = A.site_quat[0], b = A.site_quat[1], c = A.site_quat[2], d = A.site_quat[3];
    const float sw = w*a - x*b - y*c - z*d, sx = w*b + x*a + y*d - z*c, sy = w*c - x*d + y*a + z*b, sz = w*d + x*c - y*b + z*a;
    const float S[9] = {sw*sw + sx*sx - sy*sy - sz*sz, 2*(sx*sy - sw*sz), 2*(sx*sz + sw*sy), 2*(sx*sy + sw*sz), sw*sw - sx*sx + sy*sy - sz*sz,
                        2*(sy*sz - sw*sx), 2*(sx*sz - sw*sy), 2*(sy*sz + sw*sx), sw*sw - sx*sx - sy*sy + sz*sz};
    float sp[3];
#pragma unroll
    for (int k = 0; k < 3; k++) sp[k] = bp[k] + B[3*k] * A.site_pos[0] + B[3*k+1] * A.site_pos[1] + B[3*k+2] * A.site_pos[2];
    const float pw[3] = {sp[0] + S[0]*p[0] + S[1]*p[1] + S[2]*p[2], sp[1] + S[3]*p[0] + S[4]*p[1] + S[5]*p[2], sp[2] + S[6]*p[0] + S[7]*p[1] + S[8]*p[2]};
    const float vw[3] = {S[0]*v[0] + S[1]*v[1] + S[2]*v[2], S[3]*v[0] + S[4]*v[1] + S[5]*v[2], S[6]*v[0] + S[7]*v[1] + S[8]*v[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) { p[k] = pw[k]; v[k] = vw[k]; }
  }
  const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
  const bool valid = vv > 0.0f && vv < 3.0e38f;      // a zero (or non-finite) direction sees nothing
  const unsigned slotmask = A.slot_mask ? A.slot_mask[env] : 0u;
  const float* const gsize = A.size + (size_t)env * (size_t)A.size_stride;

  float best = -1.0f; int bestg = -1;
  for (int base = 0; base < A.ngeom; base += RAY_PASS) {
    __syncthreads();
    const int g = base + lane;
    if (g < A.ngeom) {       // stage geom g of this env
      float* rec = s_rec + lane * RAY_REC;
      const int4 gi = A.ginfo[g];
      const float* gp = A.gpos + ((size_t)row * A.ngeom + g) * 3;
      const float* gm = A.gmat + ((size_t)row * A.ngeom + g) * 9;
#pragma unroll
      for (int k = 0; k < 3; k++) rec[k] = gp[k];
#pragma unroll
      for (int k = 0; k < 9; k++) rec[3 + k] = gm[k];
      const float s0 = gsize[3*g], s1 = gsize[3*g + 1], s2 = gsize[3*g + 2];
      rec[12] = s0; rec[13] = s1; rec[14] = s2;
      float rb = 0.0f;
      if (gi.x == MJH_GEOM_SPHERE) rb = s0;
      else if (gi.x == MJH_GEOM_CAPSULE) rb = s0 + s1;
      else if (gi.x == MJH_GEOM_ELLIPSOID) rb = fmaxf(s0, fmaxf(s1, s2));
      else if (gi.x == MJH_GEOM_CYLINDER) rb = sqrtf(s0*s0 + s1*s1);
      else if (gi.x == MJH_GEOM_BOX) rb = sqrtf(s0*s0 + s1*s1 + s2*s2);
      else if (gi.x == MJH_GEOM_MESH) rb = A.mesh[gi.w].rbound;      // (of the model's mesh_vert: per-env sizes do not rescale a mesh, in the narrow phase neither)
      rec[15] = rb * 1.001f;     // (the reject below must never cost a hit: a sphere a little larger than the geom's)
      const bool slot_off = gi.y >= A.sbase && gi.y - A.sbase < 32 && ((slotmask >> (gi.y - A.sbase)) & 1u);
      const bool visible = gi.x >= 0 && gi.y != A.bodyexclude && (A.flg_static || !gi.z) && !slot_off;
      rec[16] = __int_as_float(visible ? gi.x : -1);
      rec[17] = __int_as_float(gi.w);
      rec[18] = __int_as_float(g);
      rec[19] = 0.0f;
    }
    __syncthreads();
    const int cnt = min(RAY_PASS, A.ngeom - base);
    for (int j = 0; j < cnt; j++) {
      const float* rec = s_rec + j * RAY_REC;
      const int type = __builtin_amdgcn_readfirstlane(__float_as_int(rec[16]));
      if (type < 0) continue;
      // the ray in the geom's frame
      const float d[3] = {p[0] - rec[0], p[1] - rec[1], p[2] - rec[2]};
      const float lp[3] = {rec[3]*d[0] + rec[6]*d[1] + rec[9]*d[2], rec[4]*d[0] + rec[7]*d[1] + rec[10]*d[2], rec[5]*d[0] + rec[8]*d[1] + rec[11]*d[2]};
      const float lv[3] = {rec[3]*v[0] + rec[6]*v[1] + rec[9]*v[2], rec[4]*v[0] + rec[7]*v[1] + rec[10]*v[2], rec[5]*v[0] + rec[8]*v[1] + rec[11]*v[2]};
      const float sz[3] = {rec[12], rec[13], rec[14]};
      float x = -1.0f;
      if (type >= MJH_GEOM_SPHERE) {
        // bounding-sphere reject: the origin outside the sphere and the ray pointing away from it, or passing it by
        const float rb = rec[15];
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
              const int mid = __builtin_amdgcn_readfirstlane(__float_as_int(rec[17]));
              const RayMesh Mh = A.mesh[mid];
              x = ray_convex(lp, lv, A.planes + Mh.adr, Mh.num);
            } break;
            default: break;
          }
        }
      } else if (valid) {
        if (type == MJH_GEOM_PLANE) x = ray_plane(lp, lv, sz);
        else {
          const int hid = __builtin_amdgcn_readfirstlane(__float_as_int(rec[17]));
          const RayHField H = A.hf[hid];
          x = ray_hfield(lp, lv, H, A.hf_data + H.adr);
        }
      }
      if (x >= 0.0f && (bestg < 0 || x < best)) { best = x; bestg = __float_as_int(rec[18]); }
    }
  }
  if (A.cutoff > 0.0f && best > A.cutoff) bestg = -1;      // rangefinder cutoff: a hit beyond it is a miss
  if (bestg < 0) best = -1.0f;
  if (live) {
    const size_t o = (size_t)row * (size_t)A.nray + (size_t)ray;
    A.dist[o] = best; A.geomid[o] = bestg;
  }
}

hipError_t mjh_launch_ray(hipStream_t st, const RayArgs& A) {
  const long long ntile = ((long long)A.nray + RAY_TILE - 1) / RAY_TILE, blocks = ntile * (long long)A.n;
  if (A.n <= 0 || A.nray <= 0 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mjh_ray_kernel, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  return hipGetLastError();
}
