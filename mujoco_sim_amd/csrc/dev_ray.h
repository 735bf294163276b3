// dev_ray.h — batched ray casting (mj_ray semantics): the launch descriptor shared by the host side (engine.hip) and the kernel
// (ray.hip), and the fp32 ray-geom intersections in the geom's own frame.  gfx950 only.
//
// Every intersection takes the ray origin p and direction v in the geom frame (v NOT normalised) and returns the smallest x >= 0 with
// p + x v on the geom's surface, or -1.  Quadratics are solved about the point of closest approach (x = tc -+ sqrt(h2 / a) with
// h2 = r^2 - |p + tc v|^2): the discriminant b^2 - a c of the textbook form cancels in fp32 once the origin is a few radii away.
#pragma once
#include <hip/hip_runtime.h>

#define RAY_TILE 64   // rays per workgroup: one wavefront, one ray per lane
#define RAY_PASS 64   // geom records one staging pass holds (one geom per lane)
#define RAY_REC 20    // floats of a record: [0..2] world position, [3..11] rotation (row-major, world = R local), [12..14] the env's size,
                      // [15] bounding radius, [16] type (int; -1: invisible in this env), [17] hfield id / mesh id (int), [18] geom id (int), [19] pad

struct RayHField { int nrow, ncol, adr, pad; float size[4]; };   // size: radius_x, radius_y, elevation_z, base_z

struct RayMesh { int adr, num; float rbound, pad; };              // a mesh asset's planes [adr, adr + num) of RayArgs::planes; bounding radius of its vertices

struct RayArgs {
  const float *gpos, *gmat;        // geom poses of the n envs as the position stage exported them: [n][3 ngeom], [n][9 ngeom]
  const float *xpos, *xquat;       // body poses [n][3 nbody], [n][4 nbody] (site >= 0 only)
  const float* size; long long size_stride;   // geom sizes: row of env `e` at size + e * size_stride (per-env tables), or stride 0 (the shared model)
  const unsigned* slot_mask; int sbase;       // spawn / destroy slots: bit b of slot_mask[env] = body sbase + b is inactive (null: none)
  const int4* ginfo;               // [ngeom]: x type (-1: no ray sees it: hfield without an asset, mesh in mesh mode 0 or without planes), y body,
                                   // z 1 = static body, w hfield id / mesh id
  const RayHField* hf; const float* hf_data;
  const RayMesh* mesh; const float4* planes;   // mesh mode 1: [nmesh], [nmeshplane] (n.x, n.y, n.z, d: unit outward normal, inside is n.x <= d)
  const float *pnt, *vec;          // [nray][3], or [n][nray][3] with per_env
  float* dist; int* geomid;        // [n][nray]
  int env0, n, nray, ngeom, nbody;
  int per_env, bodyexclude, flg_static;
  float cutoff;
  int site_body; float site_pos[3], site_quat[4];   // site frame in its body (site_body < 0: rays are given in the world frame)
};

hipError_t mjh_launch_ray(hipStream_t st, const RayArgs& A);   // ray.hip

#ifdef __HIPCC__
#define RDEV __host__ __device__ __forceinline__

RDEV float ray_pick(float best, float x) { return (x >= 0.0f && (best < 0.0f || x < best)) ? x : best; }

// roots of |p + x v|^2 = r^2 restricted to the first `dim` coordinates (3: sphere, 2: circle in the xy plane); false: none
RDEV bool ray_quadratic(const float* p, const float* v, int dim, float r, float& x0, float& x1) {
  const float a = v[0]*v[0] + v[1]*v[1] + (dim == 3 ? v[2]*v[2] : 0.0f);
  if (!(a > 1e-30f)) return false;
  const float tc = -(p[0]*v[0] + p[1]*v[1] + (dim == 3 ? p[2]*v[2] : 0.0f)) / a;
  const float qx = p[0] + tc * v[0], qy = p[1] + tc * v[1], qz = dim == 3 ? p[2] + tc * v[2] : 0.0f;
  const float h2 = r * r - (qx*qx + qy*qy + qz*qz);
  if (h2 < 0.0f) return false;
  const float h = sqrtf(h2 / a);
  x0 = tc - h; x1 = tc + h;
  return true;
}

RDEV float ray_plane(const float* p, const float* v, const float* s) {
  if (!(v[2] < 0.0f)) return -1.0f;              // front face only: the ray has to come down onto the +z side
  const float x = -p[2] / v[2];
  if (!(x >= 0.0f)) return -1.0f;
  const float hx = p[0] + x * v[0], hy = p[1] + x * v[1];
  if ((s[0] > 0.0f && fabsf(hx) > s[0]) || (s[1] > 0.0f && fabsf(hy) > s[1])) return -1.0f;
  return x;
}

RDEV float ray_sphere(const float* p, const float* v, float r) {
  float x0, x1;
  if (!ray_quadratic(p, v, 3, r, x0, x1)) return -1.0f;
  return ray_pick(ray_pick(-1.0f, x0), x1);
}

RDEV float ray_ellipsoid(const float* p, const float* v, const float* s) {
  const float ps[3] = {p[0] / s[0], p[1] / s[1], p[2] / s[2]}, vs[3] = {v[0] / s[0], v[1] / s[1], v[2] / s[2]};
  return ray_sphere(ps, vs, 1.0f);
}

// radius s[0], half length s[1] along z: the side where |z| <= s[1], the half spheres beyond
RDEV float ray_capsule(const float* p, const float* v, const float* s) {
  float best = -1.0f, x0, x1;
  if (ray_quadratic(p, v, 2, s[0], x0, x1)) {
    if (fabsf(p[2] + x0 * v[2]) <= s[1]) best = ray_pick(best, x0);
    if (fabsf(p[2] + x1 * v[2]) <= s[1]) best = ray_pick(best, x1);
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    const float sg = k ? -1.0f : 1.0f;
    const float pc[3] = {p[0], p[1], p[2] - sg * s[1]};
    if (ray_quadratic(pc, v, 3, s[0], x0, x1)) {
      if (sg * (pc[2] + x0 * v[2]) >= 0.0f) best = ray_pick(best, x0);
      if (sg * (pc[2] + x1 * v[2]) >= 0.0f) best = ray_pick(best, x1);
    }
  }
  return best;
}

// radius s[0], half length s[1], flat caps
RDEV float ray_cylinder(const float* p, const float* v, const float* s) {
  float best = -1.0f, x0, x1;
  if (ray_quadratic(p, v, 2, s[0], x0, x1)) {
    if (fabsf(p[2] + x0 * v[2]) <= s[1]) best = ray_pick(best, x0);
    if (fabsf(p[2] + x1 * v[2]) <= s[1]) best = ray_pick(best, x1);
  }
  if (v[2] != 0.0f) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const float x = ((k ? -s[1] : s[1]) - p[2]) / v[2];
      const float hx = p[0] + x * v[0], hy = p[1] + x * v[1];
      if (hx*hx + hy*hy <= s[0]*s[0]) best = ray_pick(best, x);
    }
  }
  return best;
}

// slabs: the ray is inside the box for x in [lo, hi]; false: never
RDEV bool ray_slabs(const float* p, const float* v, const float* bmin, const float* bmax, float& lo, float& hi) {
  lo = -3.0e38f; hi = 3.0e38f;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (v[k] != 0.0f) {
      const float inv = 1.0f / v[k];
      const float a = (bmin[k] - p[k]) * inv, b = (bmax[k] - p[k]) * inv;
      lo = fmaxf(lo, fminf(a, b)); hi = fminf(hi, fmaxf(a, b));
    } else if (p[k] < bmin[k] || p[k] > bmax[k]) return false;
  }
  return lo <= hi;
}

RDEV float ray_box(const float* p, const float* v, const float* s) {
  const float bmin[3] = {-s[0], -s[1], -s[2]};
  float lo, hi;
  if (!ray_slabs(p, v, bmin, s, lo, hi) || hi < 0.0f) return -1.0f;
  return lo >= 0.0f ? lo : hi;       // an origin inside the box hits the far face
}

// Convex polyhedron given by its n facet planes (planes[k] = unit outward normal, offset d; inside is n.x <= d): the ray is clipped
// against the half spaces.  With den = n.v and num = d - n.p a plane the ray runs towards from inside (den > 0) lowers the exit, one it
// enters through (den < 0) raises the entry, and a ray parallel to a plane and outside it (den == 0, num < 0) misses.  The entry if it
// is >= 0, else the exit (an origin inside hits the far surface, like the other bounded types).  n and the address of the planes
// are wave-uniform in the kernel: the plane reads are scalar loads and the loop a scalar branch, a lane carries lo, hi and the two dot
// products.  Planes go four at a time (one 64-byte scalar load); on the device the loop ends after a group once no lane of the wave
// has lo <= hi left.  The engine pads every mesh's planes to a multiple of four with (0, 0, 0, 1) — den = 0, num = 1: no effect —, so
// the tail loop is the host's.
RDEV void ray_clip(const float* p, const float* v, const float4 pl, float& lo, float& hi) {
  const float den = pl.x * v[0] + pl.y * v[1] + pl.z * v[2];
  const float num = pl.w - (pl.x * p[0] + pl.y * p[1] + pl.z * p[2]);
  const float t = num / (den != 0.0f ? den : 1.0f);      // (selects, not branches: the lanes of a wave disagree on the sign of den at most planes)
  hi = den > 0.0f ? fminf(hi, t) : hi;
  lo = den < 0.0f ? fmaxf(lo, t) : lo;
  hi = (den == 0.0f && num < 0.0f) ? -3.0e38f : hi;
}

RDEV float ray_convex(const float* p, const float* v, const float4* __restrict__ planes, int n) {
  float lo = -3.0e38f, hi = 3.0e38f;
  int k = 0;
  for (; k + 4 <= n; k += 4) {
#pragma unroll
    for (int j = 0; j < 4; j++) ray_clip(p, v, planes[k + j], lo, hi);
#ifdef __HIP_DEVICE_COMPILE__
    if (__builtin_amdgcn_ballot_w64(lo <= hi) == 0) return -1.0f;      // (wave-uniform: every lane has missed)
#endif
  }
  for (; k < n; k++) ray_clip(p, v, planes[k], lo, hi);
  if (!(lo <= hi)) return -1.0f;
  return lo >= 0.0f ? lo : (hi >= 0.0f ? hi : -1.0f);
}

// Height field: the solid the prism narrow phase collides (step_kernel.h: hfield_pair) — over grid cell (r, c) the two triangles
// (r,c) (r+1,c+1) (r,c+1) and (r,c) (r+1,c+1) (r+1,c), down to z = -size[3] — hit at its nearest surface from any side: the top
// triangles (two-sided: an origin inside the solid leaves through them), the four side walls below the terrain and the base.
// The ray is clipped to the field's box first; only the cells under the clipped segment are visited, column strip by column strip.
// A ray never passes between two cells: see the tolerance of the walk in ray_hfield.
RDEV float ray_hfield_height(const RayHField& H, const float* __restrict__ hd, float x, float y) {
  const float dx = 2.0f * H.size[0] / (float)(H.ncol - 1), dy = 2.0f * H.size[1] / (float)(H.nrow - 1);
  const float fx = fminf(fmaxf((x + H.size[0]) / dx, 0.0f), (float)(H.ncol - 1)), fy = fminf(fmaxf((y + H.size[1]) / dy, 0.0f), (float)(H.nrow - 1));
  const int c = min((int)fx, H.ncol - 2), r = min((int)fy, H.nrow - 2);
  const float u = fx - (float)c, w = fy - (float)r;
  const float z00 = hd[r * H.ncol + c], z01 = hd[r * H.ncol + c + 1], z10 = hd[(r + 1) * H.ncol + c], z11 = hd[(r + 1) * H.ncol + c + 1];
  const float h = u >= w ? z00 + u * (z01 - z00) + w * (z11 - z01) : z00 + w * (z10 - z00) + u * (z11 - z10);
  return h * H.size[2];
}

RDEV float ray_hfield(const float* p, const float* v, const RayHField& H, const float* __restrict__ hd) {
  const float sx = H.size[0], sy = H.size[1], sz = H.size[2], sb = H.size[3];
  const float bmin[3] = {-sx, -sy, -sb}, bmax[3] = {sx, sy, sz};
  float t0, t1;
  if (!ray_slabs(p, v, bmin, bmax, t0, t1) || t1 < 0.0f) return -1.0f;
  t0 = fmaxf(t0, 0.0f);
  float best = -1.0f;
  // base
  if (v[2] != 0.0f) {
    const float x = (-sb - p[2]) / v[2];
    if (fabsf(p[0] + x * v[0]) <= sx && fabsf(p[1] + x * v[1]) <= sy) best = ray_pick(best, x);
  }
  // side walls, up to the terrain's edge
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ax = k >> 1;                       // 0: the walls x = -+sx, 1: y = -+sy
    const float w = (k & 1) ? 1.0f : -1.0f;
    const float va = ax ? v[1] : v[0], pa = ax ? p[1] : p[0], sa = ax ? sy : sx, so = ax ? sx : sy;
    if (va != 0.0f) {
      const float x = (w * sa - pa) / va;
      const float o = ax ? p[0] + x * v[0] : p[1] + x * v[1], z = p[2] + x * v[2];
      if (x >= 0.0f && fabsf(o) <= so && z >= -sb) {
        const float h = ax ? ray_hfield_height(H, hd, o, w * sa) : ray_hfield_height(H, hd, w * sa, o);
        if (z <= h) best = ray_pick(best, x);
      }
    }
  }
  // top triangles of the cells under the segment [t0, t1].  Everything that places the ray on the grid comes from ONE pair of
  // expressions, the grid coordinates gu + x ud (column line c where it equals c) and gw + x wd (row line r): the strips and rows to
  // visit and a cell's u, w in [0, 1] alike, so a ray on a grid line is never rounded one way when the cell is chosen and the other
  // way when the triangle is tested.  The rounding of a grid coordinate grows with its size — half an ulp of the index per operation,
  // 4e-6 at index 33 — so the tolerance does too: 4 ulps of the largest operand (|gu| + ncol: the origin may be far outside).  Within
  // it of a line the neighbouring strip / row is visited as well and a triangle takes the point; the terrain is continuous, so the
  // neighbour's plane that far past its edge is off by the tolerance times a height difference of the cell, below fp32 resolution
  // of the distance.
  const int nc = H.ncol, nr = H.nrow;
  const float dx = 2.0f * sx / (float)(nc - 1), dy = 2.0f * sy / (float)(nr - 1);
  const float gu = (p[0] + sx) / dx, gw = (p[1] + sy) / dy, ud = v[0] / dx, wd = v[1] / dy;
  const float tolu = 4.8e-7f * (fabsf(gu) + (float)nc), tolw = 4.8e-7f * (fabsf(gw) + (float)nr);
  const float ua = gu + t0 * ud, ub = gu + t1 * ud;
  const int c0 = (int)fminf(fmaxf(floorf(fminf(ua, ub) - tolu), 0.0f), (float)(nc - 2));
  const int c1 = (int)fminf(fmaxf(floorf(fmaxf(ua, ub) + tolu), 0.0f), (float)(nc - 2));
  // (a strip taken tolu wider moves the ends of the segment over it by tolu |wd / ud| rows)
  const float rtol = v[0] != 0.0f ? tolw + tolu * fabsf(wd / ud) : tolw;
  for (int c = c0; c <= c1; c++) {
    // the part [ta, tb] of the segment over this strip of columns (all of it when the ray runs along the strip)
    float ta = t0, tb = t1;
    if (v[0] != 0.0f) {
      const float a = ((float)c - gu) / ud, b = ((float)(c + 1) - gu) / ud;
      ta = fmaxf(ta, fminf(a, b)); tb = fminf(tb, fmaxf(a, b));
    }
    if (ta > tb) ta = tb = 0.5f * (ta + tb);      // (a strip the segment only touches within the tolerance)
    const float wa = gw + ta * wd, wb = gw + tb * wd;
    const int r0 = (int)fminf(fmaxf(floorf(fminf(wa, wb) - rtol), 0.0f), (float)(nr - 2));
    const int r1 = (int)fminf(fmaxf(floorf(fmaxf(wa, wb) + rtol), 0.0f), (float)(nr - 2));
    for (int r = r0; r <= r1; r++) {
      const float z00 = hd[r * nc + c] * sz, z01 = hd[r * nc + c + 1] * sz, z10 = hd[(r + 1) * nc + c] * sz, z11 = hd[(r + 1) * nc + c + 1] * sz;
      const float u0 = gu - (float)c, w0 = gw - (float)r;      // cell coordinates of the origin
#pragma unroll
      for (int k = 0; k < 2; k++) {
        // z = z00 + u A + w B over the triangle: first u >= w, second w >= u
        const float A = k ? z11 - z10 : z01 - z00, B = k ? z10 - z00 : z11 - z01;
        const float den = v[2] - ud * A - wd * B;
        if (den == 0.0f) continue;
        const float x = (z00 + u0 * A + w0 * B - p[2]) / den;
        const float u = (gu + x * ud) - (float)c, w = (gw + x * wd) - (float)r;
        const bool in = k ? (w >= u - (tolu + tolw) && u >= -tolu && w <= 1.0f + tolw) : (u >= w - (tolu + tolw) && w >= -tolw && u <= 1.0f + tolu);
        if (in) best = ray_pick(best, x);
      }
    }
  }
  return best;
}
#endif
