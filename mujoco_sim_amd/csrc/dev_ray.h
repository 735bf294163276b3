// dev_ray.h — what the ray kernel (ray.hip) and the kernels that trace per tile (depth.hip, scan.hip, heightscan.hip, light.hip) share:
// the scene descriptor the host side (engine.hip) fills, the fp32 ray-geom intersections in the geom's own frame, and the code that
// takes a ray through an env's geoms — the frame composition, the verdict on a geom, the staged record, the walk over the records,
// the compacting staging pass (ray_stage) and the launch (ray_launch).  All but the last two is __host__ __device__: tests/ray_host
// builds it for the CPU and checks the very code the kernels run (the staging pass is wave code: the host tests stage sequentially).
// gfx950 only.
//
// Every intersection takes the ray origin p and direction v in the geom frame (v NOT normalised) and returns the smallest x >= 0 with
// p + x v on the geom's surface, or -1.  Quadratics are solved about the point of closest approach (x = tc -+ sqrt(h2 / a) with
// h2 = r^2 - |p + tc v|^2): the discriminant b^2 - a c of the textbook form cancels in fp32 once the origin is a few radii away.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/mjhip.h"
#include "ray_bvh.h"

#define RAY_TILE 64   // rays per workgroup: one wavefront, one ray per lane
#define RAY_PASS 64   // geom records one staging pass holds (one geom per lane)
#define RAY_REC 20    // floats of a record (ray_store)
#define RAY_TYPE_TRIMESH 8   // internal type of a mesh geom seen as its own triangles (not a public mjh_geom value): w = mesh id, RayScene::trimesh

struct RayHField { int nrow, ncol, adr, pad; float size[4]; };   // size: radius_x, radius_y, elevation_z, base_z

struct RayMesh { int adr, num; float rbound, pad; };              // a mesh asset's planes [adr, adr + num) of RayScene::planes; bounding radius of its vertices

// what a kernel reads of the world: n envs from env0 on, as the position-stage launch exported them (engine.hip: ray_scene)
struct RayScene {
  const float *gpos, *gmat;        // geom poses of the n envs: [n][3 ngeom], [n][9 ngeom]
  const float *xpos, *xquat;       // body poses [n][3 nbody], [n][4 nbody] (null unless asked for: a site's or a camera's body)
  const float* size; long long size_stride;   // geom sizes: row of env `e` at size + e * size_stride (per-env tables), or stride 0 (the shared model)
  const unsigned* slot_mask; int sbase;       // spawn / destroy slots: bit b of slot_mask[env] = body sbase + b is inactive (null: none)
  const int4* ginfo;               // [ngeom]: x type (-1: no ray sees it: hfield without an asset, mesh in mesh mode 0 or without planes), y body,
                                   // z 1 = static body, w hfield id / mesh id
  const RayHField* hf; const float* hf_data;
  const RayMesh* mesh; const float4* planes;   // mesh mode 1: [nmesh], [nmeshplane] (n.x, n.y, n.z, d: unit outward normal, inside is n.x <= d)
  int env0, n, ngeom, nbody;
  int bodyexclude, flg_static;     // the body no ray sees (-1: none); 0: no ray sees the geoms of static bodies
  float cutoff;                    // > 0: a reported value beyond it is a miss
};

// mesh surface 1 (ray_bvh.h): [nmesh], the meshes' nodes, four float4 per triangle; all null unless the scene's geom table holds
// RAY_TYPE_TRIMESH rows.  Beside RayScene, not in it: that struct's layout is mirrored by the host tests.
struct RayTris { const RayTriMesh* mesh; const RayNode* nodes; const float4* tris; };

struct RayArgs {
  RayScene W;
  const float *pnt, *vec;          // [nray][3], or [n][nray][3] with per_env
  float* dist; int* geomid;        // [n][nray]
  int nray, per_env;
  int site_body; float site_pos[3], site_quat[4];   // site frame in its body (site_body < 0: rays are given in the world frame)
  RayTris T;
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

// a candidate x of ray_hfield (the base, a wall, a top triangle) under ray_pick's rule.  NRM: where it replaces `best` (a strictly
// smaller x, or the first one), its normal (nx, ny, nz) replaces nrm
template <bool NRM>
RDEV void ray_hfield_take(float& best, float x, float nx, float ny, float nz, float* nrm) {
  if constexpr (NRM) {
    const float nb = ray_pick(best, x);
    if (nb != best) { best = nb; nrm[0] = nx; nrm[1] = ny; nrm[2] = nz; }
  } else best = ray_pick(best, x);
}

// NRM: nrm also receives the normal of the feature that gives the returned x — the base (0, 0, -1), a wall's outward axis, or the
// geometric normal of the top triangle: over cell (r, c) triangle k is z = z00 + u A + w B with u = (X + sx) / dx - c and
// w = (Y + sy) / dy - r, so its upward normal is (-A / dx, -B / dy, 1) — in the geom frame, neither normalised nor oriented, (0, 0, 0)
// without a hit.  The instance without NRM is the code as it was before the parameter existed, token for token: the kernels' bits
// depend on it (HISTORY.md).
template <bool NRM = false>
RDEV float ray_hfield(const float* p, const float* v, const RayHField& H, const float* __restrict__ hd, float* nrm = nullptr) {
  if constexpr (NRM) nrm[0] = nrm[1] = nrm[2] = 0.0f;
  const float sx = H.size[0], sy = H.size[1], sz = H.size[2], sb = H.size[3];
  const float bmin[3] = {-sx, -sy, -sb}, bmax[3] = {sx, sy, sz};
  float t0, t1;
  if (!ray_slabs(p, v, bmin, bmax, t0, t1) || t1 < 0.0f) return -1.0f;
  t0 = fmaxf(t0, 0.0f);
  float best = -1.0f;
  // base
  if (v[2] != 0.0f) {
    const float x = (-sb - p[2]) / v[2];
    if (fabsf(p[0] + x * v[0]) <= sx && fabsf(p[1] + x * v[1]) <= sy) ray_hfield_take<NRM>(best, x, 0.0f, 0.0f, -1.0f, nrm);
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
        if (z <= h) ray_hfield_take<NRM>(best, x, ax ? 0.0f : w, ax ? w : 0.0f, 0.0f, nrm);
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
        if (in) ray_hfield_take<NRM>(best, x, -A / dx, -B / dy, 1.0f, nrm);
      }
    }
  }
  return best;
}

// a wave-uniform value read into a scalar register (the identity in a host compile)
RDEV int ray_uniform(int x) {
#ifdef __HIP_DEVICE_COMPILE__
  return __builtin_amdgcn_readfirstlane(x);
#else
  return x;
#endif
}
RDEV int ray_bits(float x) { return __builtin_bit_cast(int, x); }
RDEV float ray_float(int x) { return __builtin_bit_cast(float, x); }
static __device__ __forceinline__ float uniform(float x) { return ray_float(ray_uniform(ray_bits(x))); }

// A mesh's own triangles (ray_bvh.h: the records, the threaded BVH and the slack).  ray_tri is Moeller-Trumbore in fp32, two-sided:
// with P = v x e2, det = e1.P, T = p - a, Q = T x e1 the hit is u = T.P / det, w = v.Q / det, x = e2.Q / det.
//   parallel: |det| <= 2^-22 |e1|_1 |e2|_1 |v|_1 is rounding noise of the three products of det (two ulps of their scale): a miss.
//   edges: u >= -eu, w >= -ew, u + w <= 1 + eu + ew with eu = 2^-20 L |v|_1 |e2|_1 / |det|, ew likewise with |e1|_1, L = |p|_1 + R1 (R1:
//     the mesh's largest corner 1-norm).  Eight ulps of the operand scale of the numerator: T carries half an ulp of L from the
//     subtraction and another from the stored corner (1.2e-7 L |P|_1), a component of P three roundings of |v||e2| (0.9e-7 |v|_1 |e2|_1
//     each), the dot product three more of its terms (2e-7), det the same relative to |e1|_1 <= L (3e-7, times u <= 1): 7.4e-7 in
//     all in the worst case, under 2^-20 = 9.5e-7.  Two triangles that share an edge store it from different corners (a + e1 here,
//     a' + e2' there): that is the stored-corner term.  So on a shared edge or vertex at least one of the neighbours takes the point.
//   box: the hit point p + x v, as fp32 computes it, must lie in the triangle's own box widened by sp = 2^-21 |p|_1 (the record's
//     box carries 2^-21 R1 already).  This bounds what the edge slack can accept for a grazing ray (eu grows as 1 / det), and it is
//     what makes pruning exact (ray_bvh.h): an accepted x lies inside every enclosing node's widened box.
// sp, L and vn = |v|_1 are the ray's, computed once per geom.
RDEV float ray_tri(const float* p, const float* v, float vn, float L, float sp, const float4 q0, const float4 q1, const float4 q2, const float4 q3) {
  const float e1[3] = {q1.x, q1.y, q1.z}, e2[3] = {q2.x, q2.y, q2.z};
  const float n1 = q0.w, n2 = fabsf(e2[0]) + fabsf(e2[1]) + fabsf(e2[2]);
  const float P[3] = {v[1]*e2[2] - v[2]*e2[1], v[2]*e2[0] - v[0]*e2[2], v[0]*e2[1] - v[1]*e2[0]};
  const float det = e1[0]*P[0] + e1[1]*P[1] + e1[2]*P[2];
  if (!(fabsf(det) > 2.38418579e-7f * n1 * n2 * vn)) return -1.0f;
  const float inv = 1.0f / det;
  const float T[3] = {p[0] - q0.x, p[1] - q0.y, p[2] - q0.z};
  const float Q[3] = {T[1]*e1[2] - T[2]*e1[1], T[2]*e1[0] - T[0]*e1[2], T[0]*e1[1] - T[1]*e1[0]};
  const float u = (T[0]*P[0] + T[1]*P[1] + T[2]*P[2]) * inv, w = (v[0]*Q[0] + v[1]*Q[1] + v[2]*Q[2]) * inv;
  const float x = (e2[0]*Q[0] + e2[1]*Q[1] + e2[2]*Q[2]) * inv;
  const float ek = 9.53674316e-7f * L * vn * fabsf(inv), eu = ek * n2, ew = ek * n1;
  const float X[3] = {p[0] + x * v[0], p[1] + x * v[1], p[2] + x * v[2]};
  const bool in = u >= -eu && w >= -ew && u + w <= 1.0f + eu + ew && x >= 0.0f;
  const bool box = X[0] >= q1.w - sp && X[1] >= q2.w - sp && X[2] >= q3.x - sp && X[0] <= q3.y + sp && X[1] <= q3.z + sp && X[2] <= q3.w + sp;
  return in && box ? x : -1.0f;
}

// The smallest x in [0, bound] with p + x v on a triangle of the mesh, or -1; bound: the ray's best hit so far (3e38: none) — x is the
// same parameter in every geom frame, so a node the ray enters beyond it holds nothing the walk would take (it replaces a record only
// for x < best).  One forward scan of the mesh's nodes (ray_bvh.h): i -> i + 1 or i -> skip > i, so it ends after at most nnode steps
// whatever the tables hold; no stack, no private array.  In the kernels the mesh is wave-uniform: i lives in a scalar register, a node
// and a triangle come by scalar loads, the subtree is skipped when NO lane of the wave wants it (a lane that did not want a leaf
// tests its triangles all the same: by the argument of ray_bvh.h it finds nothing below its bound there).  A node's slab test uses
// the reciprocal direction (+-inf for a zero component: the products are then +-inf, or NaN for an origin on the slab's face, which
// fminf / fmaxf drop: inside) and the box widened by sn = 3 sp.
// NRM: nrm also receives e1 x e2 of the triangle the scan takes (the later one of the scan on an equal x) — the geom frame, neither
// normalised nor oriented, (0, 0, 0) without a hit.  The shade kernel calls it on the one geom a pixel names with a bound a little above
// the known x; there only the lanes that hold this geom are active: the ballot sees them alone, and every one of them stays in the scan
// until it ends.  The instance without NRM is the code as it was before the parameter existed.
template <bool NRM = false>
RDEV float ray_trimesh(const float* p, const float* v, const RayTriMesh& M, const RayNode* __restrict__ nodes, const float4* __restrict__ tris, float bound, float* nrm = nullptr) {
  const float vn = fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]), pn = fabsf(p[0]) + fabsf(p[1]) + fabsf(p[2]);
  const float L = pn + M.r1, sp = RAY_SLACK * pn, sn = RAY_NODE_SLACK * sp;
  const float iv[3] = {1.0f / v[0], 1.0f / v[1], 1.0f / v[2]};
  const float pl[3] = {p[0] + sn, p[1] + sn, p[2] + sn}, ph[3] = {p[0] - sn, p[1] - sn, p[2] - sn};
  float cur = -1.0f, lim = bound;
  if constexpr (NRM) nrm[0] = nrm[1] = nrm[2] = 0.0f;
  const int n = M.nnode;
  int i = 0;
  while (i < n) {
    const RayNode N = nodes[i];
    float lo = -3.0e38f, hi = 3.0e38f;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const float a = (N.bmin[k] - pl[k]) * iv[k], b = (N.bmax[k] - ph[k]) * iv[k];
      lo = fmaxf(lo, fminf(a, b)); hi = fminf(hi, fmaxf(a, b));
    }
    const bool hit = lo <= hi && hi >= 0.0f && lo <= lim;
#ifdef __HIP_DEVICE_COMPILE__
    const bool go = __builtin_amdgcn_ballot_w64(hit) != 0;      // (wave-uniform)
#else
    const bool go = hit;
#endif
    if (!go) { i = ray_uniform(N.skip); continue; }
    const int leaf = ray_uniform(N.leaf);
    if (leaf >= 0) {
      const float4* q = tris + (size_t)4 * (size_t)(leaf >> 3);
      const int cnt = leaf & 7;
      for (int t = 0; t < cnt; t++) {
        const float4 q1 = q[4*t + 1], q2 = q[4*t + 2];
        const float x = ray_tri(p, v, vn, L, sp, q[4*t], q1, q2, q[4*t + 3]);
        if (x >= 0.0f && x <= lim) {
          cur = x; lim = x;
          if constexpr (NRM) { nrm[0] = q1.y * q2.z - q1.z * q2.y; nrm[1] = q1.z * q2.x - q1.x * q2.z; nrm[2] = q1.x * q2.y - q1.y * q2.x; }
        }
      }
    }
    i = i + 1;
  }
  return cur;
}

// ---- a ray through the geoms of an env

// world origin o[3] and rotation S[9] (row-major, world = S local) of a frame (pos, quat) given in a body (a site, a camera), from the
// body's exported world pose bp, bq.  A macro, not a function: the kernels' bits depend on it.  As an RDEV function (pos / quat as
// pointers or as references to the descriptor's arrays alike) the same expressions compile to other bits, because the compiler orders
// the operands of the quaternion product's sums differently and then fuses another product of a sum into the FMA (HISTORY.md).
#define RAY_FRAME(bp, bq, pos, quat, o, S)                                                                                             \
  do {                                                                                                                                 \
    const float *const f_bp = (bp), *const f_bq = (bq), *const f_pos = (pos), *const f_quat = (quat);                                  \
    const float w = f_bq[0], x = f_bq[1], y = f_bq[2], z = f_bq[3];                                                                    \
    const float B[9] = {w*w + x*x - y*y - z*z, 2*(x*y - w*z), 2*(x*z + w*y), 2*(x*y + w*z), w*w - x*x + y*y - z*z, 2*(y*z - w*x),      \
                        2*(x*z - w*y), 2*(y*z + w*x), w*w - x*x - y*y + z*z};                                                          \
    const float a = f_quat[0], b = f_quat[1], c = f_quat[2], d = f_quat[3];                                                            \
    const float sw = w*a - x*b - y*c - z*d, sx = w*b + x*a + y*d - z*c, sy = w*c - x*d + y*a + z*b, sz = w*d + x*c - y*b + z*a;        \
    (S)[0] = sw*sw + sx*sx - sy*sy - sz*sz; (S)[1] = 2*(sx*sy - sw*sz); (S)[2] = 2*(sx*sz + sw*sy);                                    \
    (S)[3] = 2*(sx*sy + sw*sz); (S)[4] = sw*sw - sx*sx + sy*sy - sz*sz; (S)[5] = 2*(sy*sz - sw*sx);                                    \
    (S)[6] = 2*(sx*sz - sw*sy); (S)[7] = 2*(sy*sz + sw*sx); (S)[8] = sw*sw - sx*sx - sy*sy + sz*sz;                                    \
    for (int k = 0; k < 3; k++) (o)[k] = f_bp[k] + B[3*k] * f_pos[0] + B[3*k+1] * f_pos[1] + B[3*k+2] * f_pos[2];                      \
  } while (0)

// the verdict on a geom (its ginfo row gi, its size s in the env, the env's slot mask): the type a ray sees, or -1 for a geom
// invisible in this env; rb: the radius of its bounding sphere (of a mesh: of the model's mesh_vert — per-env sizes do not rescale a
// mesh, in the narrow phase neither), a little larger than the geom's: the reject of the walk must never cost a hit.  TRI: the geom table
// may hold RAY_TYPE_TRIMESH rows (mesh surface 1); without it the function is the code it was before that type existed
template <bool TRI = false>
RDEV int ray_verdict(const RayScene& W, const int4 gi, const float* s, unsigned slotmask, float& rb, const RayTris* T = nullptr) {
  rb = 0.0f;
  if (gi.x == MJH_GEOM_SPHERE) rb = s[0];
  else if (gi.x == MJH_GEOM_CAPSULE) rb = s[0] + s[1];
  else if (gi.x == MJH_GEOM_ELLIPSOID) rb = fmaxf(s[0], fmaxf(s[1], s[2]));
  else if (gi.x == MJH_GEOM_CYLINDER) rb = sqrtf(s[0]*s[0] + s[1]*s[1]);
  else if (gi.x == MJH_GEOM_BOX) rb = sqrtf(s[0]*s[0] + s[1]*s[1] + s[2]*s[2]);
  else if (gi.x == MJH_GEOM_MESH) rb = W.mesh[gi.w].rbound;
  if constexpr (TRI) { if (gi.x == RAY_TYPE_TRIMESH) rb = T->mesh[gi.w].rbound; }      // (of the triangles' corners: the kept vertices of `mesh` are an inner approximation)
  rb *= 1.001f;
  const bool slot_off = gi.y >= W.sbase && gi.y - W.sbase < 32 && ((slotmask >> (gi.y - W.sbase)) & 1u);
  const bool visible = gi.x >= 0 && gi.y != W.bodyexclude && (W.flg_static || !gi.z) && !slot_off;
  return visible ? gi.x : -1;
}

// the record of a staged geom, RAY_REC floats: [0..2] world position, [3..11] rotation (row-major, world = R local), [12..14] the env's
// size, [15] bounding radius, [16] type (int; -1: invisible in this env), [17] hfield id / mesh id (int), [18] geom id (int), [19] pad
RDEV void ray_store(float* rec, const float* pos, const float* mat, const float* s, float rb, int type, int id, int g) {
#pragma unroll
  for (int k = 0; k < 3; k++) rec[k] = pos[k];
#pragma unroll
  for (int k = 0; k < 9; k++) rec[3 + k] = mat[k];
#pragma unroll
  for (int k = 0; k < 3; k++) rec[12 + k] = s[k];
  rec[15] = rb;
  rec[16] = ray_float(type);
  rec[17] = ray_float(id);
  rec[18] = ray_float(g);
  rec[19] = 0.0f;
}

// the walk: the world-frame ray (p, v; vv = |v|^2; valid: 0 < vv < inf) against `cnt` staged records, in their order; best / bestg
// keep the nearest hit, the earlier record on a tie.  In the kernels every lane of a wave walks the same records: the record index is
// wave-uniform, so the type switch is a scalar branch and the record reads are LDS broadcasts.  SKIP: records of type -1 occur.
// TRI: records of RAY_TYPE_TRIMESH occur (mesh surface 1).  The kernels are compiled once with and once without it, and a launch takes
// the instance without unless the scene has triangle tables: as one more case of the one switch the walk cost the scenes that have no
// such record 1.5 - 4.6 %, through the compiler's register and branch layout alone.
template <bool SKIP, bool TRI = false>
RDEV void ray_walk(const RayScene& W, const float* recs, int cnt, const float* p, const float* v, float vv, bool valid, float& best, int& bestg, const RayTris* T = nullptr) {
  for (int j = 0; j < cnt; j++) {
    const float* rec = recs + j * RAY_REC;
    const int type = ray_uniform(ray_bits(rec[16]));
    if (SKIP && type < 0) continue;
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
            const RayMesh Mh = W.mesh[ray_uniform(ray_bits(rec[17]))];
            x = ray_convex(lp, lv, W.planes + Mh.adr, Mh.num);
          } break;
          default:
            if constexpr (TRI) {
              if (type == RAY_TYPE_TRIMESH) {      // the mesh id is wave-uniform: its table row, the nodes and the triangles come by scalar loads
                const RayTriMesh Mt = T->mesh[ray_uniform(ray_bits(rec[17]))];
                x = ray_trimesh(lp, lv, Mt, T->nodes + Mt.node, T->tris + (size_t)4 * (size_t)Mt.tri, bestg < 0 ? 3.0e38f : best);
              }
            }
            break;
        }
      }
    } else if (valid) {
      if (type == MJH_GEOM_PLANE) x = ray_plane(lp, lv, sz);
      else {
        const RayHField H = W.hf[ray_uniform(ray_bits(rec[17]))];
        x = ray_hfield(lp, lv, H, W.hf_data + H.adr);
      }
    }
    if (x >= 0.0f && (bestg < 0 || x < best)) { best = x; bestg = ray_bits(rec[18]); }
  }
}

// planes and height fields are never culled: the types a tile's bound (cone, cylinder, shadow segment) may drop
RDEV bool ray_cullable(const int4 gi) { return gi.x >= MJH_GEOM_SPHERE; }

// One staging pass of the kernels that trace per tile (depth, scan, heightscan, light): the RAY_PASS geoms of env row `row` from `base`
// on, one per lane — the verdict first (type, body, bounding sphere), then the caller's own predicate, and only a survivor's record is
// read and stored.  The survivors are compacted into s_rec by ballot and a lane prefix count, in ascending geom id (so ties break as in
// ray.hip); their number is returned for ray_walk<false>.  Both barriers are inside: every lane of the wave must call it.  Device only;
// position is loaded before size and nothing is interleaved (HISTORY.md).  No floating-point arithmetic of its own.
// keep_geom(keep, gi, c, rb) -> keep: `keep` is the verdict, c the world position, rb the bounding radius.  A predicate only ever
// clears it, every clause behind `keep &&`, so nothing is evaluated for a geom the verdict dropped.  Two things about its form are
// measured, not taste (HISTORY.md, "One staging pass ..."): it takes and returns `keep` (called as `if (keep) keep = pred(...)` the
// compiler keeps one more exec mask alive across the pass, and the kernels capped at 96 scalar registers spill up to six more values to
// lanes: the height scan ran 2 % slower); and it is a lambda that captures BY VALUE ([=]) scalars and short arrays copied into locals
// (by reference the kernel's wave-uniform values reach the walk's sums as loads through the closure, the compiler orders their
// operands differently and fuses other products into the FMAs: other bits in the height scan's images).
template <bool TRI, class Keep>
static __device__ __forceinline__ int ray_stage(const RayScene& W, const RayTris* T, float* s_rec, int row, int base, int lane, unsigned slotmask, const float* gsize, Keep keep_geom) {
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
    keep = keep_geom(ray_verdict<TRI>(W, gi, s, slotmask, rb, T) >= 0, gi, c, rb);
  }
  const unsigned long long kept = __ballot(keep);
  if (keep) {      // record `number of survivors in the lanes below`
    const int slot = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(kept >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kept, 0u));
    ray_store(s_rec + slot * RAY_REC, c, W.gmat + ((size_t)row * W.ngeom + g) * 9, s, rb, gi.x, gi.w, g);
  }
  __syncthreads();
  return __popcll(kept);
}

// the launch of every kernel of these units: `blocks` workgroups of one wavefront each, refused when no grid holds that many.
// RAY_LAUNCH_TRI takes the <true> instance of a kernel template where the scene has triangle tables (T.mesh), else <false>.
template <class Args>
static inline hipError_t ray_launch(void (*kernel)(const Args), long long blocks, hipStream_t st, const Args& A) {
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(RAY_TILE), 0, st, A);
  return hipGetLastError();
}
#define RAY_LAUNCH_TRI(kernel, T, blocks, st, A) ray_launch((T).mesh ? kernel<true> : kernel<false>, blocks, st, A)
#endif
