// dev_render.h — RGB-D images (mjh_render / mjh_render_device): what the shade kernel (render.hip) adds to dev_ray.h and dev_depth.h — its
// launch descriptor, the surface normal of every geom type a ray can see, resolved on the ONE geom a depth pixel names, and the colour
// of a pixel.  The functions are __host__ __device__: tests/render_host builds them for the CPU and checks the very code the kernel
// runs.  Nothing here walks an env's geoms: the depth launch has done that, the resolve functions take a geom, the ray in the geom's
// frame and the ray parameter x of the hit, so ray.hip can take them later for mjh_ray.  gfx950 only.
//
// A normal is returned in the geom's frame, NOT normalised and NOT oriented (render_finish does both in the world frame).
#pragma once
#include <hip/hip_runtime.h>

#include "dev_depth.h"

struct ShadeArgs {
  DepthArgs D;                     // the depth launch's own descriptor: D.depth / D.geomid are read here, never written
  const float4* color;             // [ngeom] geom_rgba
  float* normal;                   // [n][height][width][3], may be null
  unsigned* rgba;                  // [n][height][width] (R, G, B, A bytes in memory order), may be null
  float ambient, diffuse;
  unsigned background;             // the packed colour of a miss
};

hipError_t mjh_launch_shade(hipStream_t st, const ShadeArgs& A);   // render.hip

#ifdef __HIPCC__
// ---- the analytic types: the normal at the hit point h (geom frame)
RDEV void normal_ellipsoid(const float* h, const float* s, float* n) {
  n[0] = h[0] / (s[0] * s[0]); n[1] = h[1] / (s[1] * s[1]); n[2] = h[2] / (s[2] * s[2]);
}
RDEV void normal_capsule(const float* h, const float* s, float* n) {
  n[0] = h[0]; n[1] = h[1]; n[2] = h[2] - fminf(fmaxf(h[2], -s[1]), s[1]);
}
// the cap where the point is further outside (or less inside) the cap's plane than the side
RDEV void normal_cylinder(const float* h, const float* s, float* n) {
  const bool cap = fabsf(h[2]) - s[1] >= sqrtf(h[0]*h[0] + h[1]*h[1]) - s[0];
  n[0] = cap ? 0.0f : h[0]; n[1] = cap ? 0.0f : h[1]; n[2] = cap ? (h[2] < 0.0f ? -1.0f : 1.0f) : 0.0f;
}
// the face whose plane the point is nearest to from inside (furthest outside): selects, no indexed array
RDEV void normal_box(const float* h, const float* s, float* n) {
  const float ex = fabsf(h[0]) - s[0], ey = fabsf(h[1]) - s[1], ez = fabsf(h[2]) - s[2];
  const bool fx = ex >= ey && ex >= ez, fy = !fx && ey >= ez;
  n[0] = fx ? (h[0] < 0.0f ? -1.0f : 1.0f) : 0.0f;
  n[1] = fy ? (h[1] < 0.0f ? -1.0f : 1.0f) : 0.0f;
  n[2] = (!fx && !fy) ? (h[2] < 0.0f ? -1.0f : 1.0f) : 0.0f;
}

// ---- the table types
// hull (mesh mode 1): the plane the hit point lies on is the one it is least inside of — the largest n.X - d; the padding planes
// (0, 0, 0, 1) give -1 and a point of the surface about 0 on its own plane.  n and the planes are wave-uniform in the kernel.
RDEV void normal_convex(const float* h, const float4* __restrict__ planes, int num, float* n) {
  float best = -3.0e38f;
  n[0] = n[1] = n[2] = 0.0f;
  for (int k = 0; k < num; k++) {
    const float4 pl = planes[k];
    const float e = pl.x * h[0] + pl.y * h[1] + pl.z * h[2] - pl.w;
    const bool take = e > best;
    best = take ? e : best; n[0] = take ? pl.x : n[0]; n[1] = take ? pl.y : n[1]; n[2] = take ? pl.z : n[2];
  }
}

// triangles (mesh surface 1): ray_trimesh's scan (dev_ray.h) that also keeps e1 x e2 of the triangle it takes — the later triangle of
// the scan on an equal x, as there.  bound: a little above the known x of the hit, so subtrees the ray enters behind it are pruned.  The
// return value is the x it found (-1: none: n stays 0).  In the kernel only the lanes that hold this geom are active: the ballot sees
// them alone, and every one of them stays in the scan until it ends.
RDEV float normal_trimesh(const float* p, const float* v, const RayTriMesh& M, const RayNode* __restrict__ nodes, const float4* __restrict__ tris, float bound, float* nrm) {
  const float vn = fabsf(v[0]) + fabsf(v[1]) + fabsf(v[2]), pn = fabsf(p[0]) + fabsf(p[1]) + fabsf(p[2]);
  const float L = pn + M.r1, sp = RAY_SLACK * pn, sn = RAY_NODE_SLACK * sp;
  const float iv[3] = {1.0f / v[0], 1.0f / v[1], 1.0f / v[2]};
  const float pl[3] = {p[0] + sn, p[1] + sn, p[2] + sn}, ph[3] = {p[0] - sn, p[1] - sn, p[2] - sn};
  float cur = -1.0f, lim = bound;
  nrm[0] = nrm[1] = nrm[2] = 0.0f;
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
    const bool go = __builtin_amdgcn_ballot_w64(hit) != 0;      // (uniform over the active lanes)
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
          nrm[0] = q1.y * q2.z - q1.z * q2.y; nrm[1] = q1.z * q2.x - q1.x * q2.z; nrm[2] = q1.x * q2.y - q1.y * q2.x;
        }
      }
    }
    i = i + 1;
  }
  return cur;
}

// height field: ray_hfield (dev_ray.h) with the normal of the feature that gives the nearest hit — the base (0, 0, -1), a wall's outward
// axis, or the geometric normal of the top triangle: over cell (r, c) triangle k is z = z00 + u A + w B with u = (X + sx) / dx - c and
// w = (Y + sy) / dy - r, so its upward normal is (-A / dx, -B / dy, 1).  The candidates come in ray_hfield's order and replace the best
// under ray_pick's rule (a strictly smaller x): the feature is the one whose x ray_hfield returned.
RDEV float normal_hfield(const float* p, const float* v, const RayHField& H, const float* __restrict__ hd, float* nrm) {
  nrm[0] = nrm[1] = nrm[2] = 0.0f;
  const float sx = H.size[0], sy = H.size[1], sz = H.size[2], sb = H.size[3];
  const float bmin[3] = {-sx, -sy, -sb}, bmax[3] = {sx, sy, sz};
  float t0, t1;
  if (!ray_slabs(p, v, bmin, bmax, t0, t1) || t1 < 0.0f) return -1.0f;
  t0 = fmaxf(t0, 0.0f);
  float best = -1.0f;
  if (v[2] != 0.0f) {
    const float x = (-sb - p[2]) / v[2];
    if (fabsf(p[0] + x * v[0]) <= sx && fabsf(p[1] + x * v[1]) <= sy) {
      const float nb = ray_pick(best, x);
      if (nb != best) { best = nb; nrm[0] = 0.0f; nrm[1] = 0.0f; nrm[2] = -1.0f; }
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ax = k >> 1;
    const float w = (k & 1) ? 1.0f : -1.0f;
    const float va = ax ? v[1] : v[0], pa = ax ? p[1] : p[0], sa = ax ? sy : sx, so = ax ? sx : sy;
    if (va != 0.0f) {
      const float x = (w * sa - pa) / va;
      const float o = ax ? p[0] + x * v[0] : p[1] + x * v[1], z = p[2] + x * v[2];
      if (x >= 0.0f && fabsf(o) <= so && z >= -sb) {
        const float h = ax ? ray_hfield_height(H, hd, o, w * sa) : ray_hfield_height(H, hd, w * sa, o);
        if (z <= h) {
          const float nb = ray_pick(best, x);
          if (nb != best) { best = nb; nrm[0] = ax ? 0.0f : w; nrm[1] = ax ? w : 0.0f; nrm[2] = 0.0f; }
        }
      }
    }
  }
  const int nc = H.ncol, nr = H.nrow;
  const float dx = 2.0f * sx / (float)(nc - 1), dy = 2.0f * sy / (float)(nr - 1);
  const float gu = (p[0] + sx) / dx, gw = (p[1] + sy) / dy, ud = v[0] / dx, wd = v[1] / dy;
  const float tolu = 4.8e-7f * (fabsf(gu) + (float)nc), tolw = 4.8e-7f * (fabsf(gw) + (float)nr);
  const float ua = gu + t0 * ud, ub = gu + t1 * ud;
  const int c0 = (int)fminf(fmaxf(floorf(fminf(ua, ub) - tolu), 0.0f), (float)(nc - 2));
  const int c1 = (int)fminf(fmaxf(floorf(fmaxf(ua, ub) + tolu), 0.0f), (float)(nc - 2));
  const float rtol = v[0] != 0.0f ? tolw + tolu * fabsf(wd / ud) : tolw;
  for (int c = c0; c <= c1; c++) {
    float ta = t0, tb = t1;
    if (v[0] != 0.0f) {
      const float a = ((float)c - gu) / ud, b = ((float)(c + 1) - gu) / ud;
      ta = fmaxf(ta, fminf(a, b)); tb = fminf(tb, fmaxf(a, b));
    }
    if (ta > tb) ta = tb = 0.5f * (ta + tb);
    const float wa = gw + ta * wd, wb = gw + tb * wd;
    const int r0 = (int)fminf(fmaxf(floorf(fminf(wa, wb) - rtol), 0.0f), (float)(nr - 2));
    const int r1 = (int)fminf(fmaxf(floorf(fmaxf(wa, wb) + rtol), 0.0f), (float)(nr - 2));
    for (int r = r0; r <= r1; r++) {
      const float z00 = hd[r * nc + c] * sz, z01 = hd[r * nc + c + 1] * sz, z10 = hd[(r + 1) * nc + c] * sz, z11 = hd[(r + 1) * nc + c + 1] * sz;
      const float u0 = gu - (float)c, w0 = gw - (float)r;
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const float A = k ? z11 - z10 : z01 - z00, B = k ? z10 - z00 : z11 - z01;
        const float den = v[2] - ud * A - wd * B;
        if (den == 0.0f) continue;
        const float x = (z00 + u0 * A + w0 * B - p[2]) / den;
        const float u = (gu + x * ud) - (float)c, w = (gw + x * wd) - (float)r;
        const bool in = k ? (w >= u - (tolu + tolw) && u >= -tolu && w <= 1.0f + tolw) : (u >= w - (tolu + tolw) && w >= -tolw && u <= 1.0f + tolu);
        if (in) {
          const float nb = ray_pick(best, x);
          if (nb != best) { best = nb; nrm[0] = -A / dx; nrm[1] = -B / dy; nrm[2] = 1.0f; }
        }
      }
    }
  }
  return best;
}

// ---- the normal of geom g's surface where the world-frame ray (p, v) meets it at parameter x: the geom's type / table row gi
// (RayScene::ginfo), world pose (pos, mat: row-major, world = mat local) and size s in the env.  nw: world frame, not normalised,
// not oriented; (0, 0, 0) for a type no ray sees.  The ray in the geom's frame is formed as ray_walk forms it.  In the kernel gi, pos,
// mat and s are wave-uniform: the switch is a scalar branch and the table reads are scalar loads.
RDEV void render_normal(const RayScene& W, const RayTris& T, const int4 gi, const float* pos, const float* mat, const float* s,
                        const float* p, const float* v, float x, float* nw) {
  const float d[3] = {p[0] - pos[0], p[1] - pos[1], p[2] - pos[2]};
  const float lp[3] = {mat[0]*d[0] + mat[3]*d[1] + mat[6]*d[2], mat[1]*d[0] + mat[4]*d[1] + mat[7]*d[2], mat[2]*d[0] + mat[5]*d[1] + mat[8]*d[2]};
  const float lv[3] = {mat[0]*v[0] + mat[3]*v[1] + mat[6]*v[2], mat[1]*v[0] + mat[4]*v[1] + mat[7]*v[2], mat[2]*v[0] + mat[5]*v[1] + mat[8]*v[2]};
  const float h[3] = {lp[0] + x * lv[0], lp[1] + x * lv[1], lp[2] + x * lv[2]};
  float n[3] = {0.0f, 0.0f, 0.0f};
  switch (gi.x) {
    case MJH_GEOM_PLANE: n[2] = 1.0f; break;
    case MJH_GEOM_HFIELD: {
      const RayHField H = W.hf[gi.w];
      normal_hfield(lp, lv, H, W.hf_data + H.adr, n);
    } break;
    case MJH_GEOM_SPHERE: n[0] = h[0]; n[1] = h[1]; n[2] = h[2]; break;
    case MJH_GEOM_CAPSULE: normal_capsule(h, s, n); break;
    case MJH_GEOM_ELLIPSOID: normal_ellipsoid(h, s, n); break;
    case MJH_GEOM_CYLINDER: normal_cylinder(h, s, n); break;
    case MJH_GEOM_BOX: normal_box(h, s, n); break;
    case MJH_GEOM_MESH: {
      const RayMesh Mh = W.mesh[gi.w];
      normal_convex(h, W.planes + Mh.adr, Mh.num, n);
    } break;
    case RAY_TYPE_TRIMESH:
      if (T.mesh) {
        const RayTriMesh Mt = T.mesh[gi.w];
        normal_trimesh(lp, lv, Mt, T.nodes + Mt.node, T.tris + (size_t)4 * (size_t)Mt.tri, x + 1e-3f * fabsf(x) + 1e-30f, n);
      }
      break;
    default: break;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) nw[k] = mat[3*k] * n[0] + mat[3*k+1] * n[1] + mat[3*k+2] * n[2];
}

// unit length and orientation towards the ray's origin (n . v <= 0); returns |n . v^| (v^ the unit direction, vv = |v|^2) clamped to
// [0, 1], 1 where it is not a number.  A zero or non-finite normal becomes (0, 0, 0).
RDEV float render_finish(float* n, const float* v, float vv) {
  const float nn = n[0]*n[0] + n[1]*n[1] + n[2]*n[2];
  const bool ok = nn > 0.0f && nn < 3.0e38f;
  const float inv = ok ? 1.0f / sqrtf(nn) : 0.0f;
  const float dot = (n[0]*v[0] + n[1]*v[1] + n[2]*v[2]) * inv;
  const float sg = dot > 0.0f ? -inv : inv;
#pragma unroll
  for (int k = 0; k < 3; k++) n[k] = ok ? n[k] * sg : 0.0f;
  const float c = fabsf(dot) / sqrtf(vv);
  return c <= 1.0f ? c : 1.0f;
}

// a channel: (int)(255 min(1, c) + 0.5) with the product and the sum rounded separately (no FMA: the value is defined bit for bit)
RDEV unsigned render_level(float c) {
#pragma clang fp contract(off)
  const float m = 255.0f * fminf(1.0f, c);
  return (unsigned)(int)(m + 0.5f);
}
RDEV unsigned render_pack(float r, float g, float b, float a) {
  return render_level(r) | (render_level(g) << 8) | (render_level(b) << 16) | (render_level(a) << 24);
}
// the colour of a hit: the geom's r, g, b times shade = ambient + diffuse * ndv, alpha 255
RDEV unsigned render_color(const float4 col, float ambient, float diffuse, float ndv) {
#pragma clang fp contract(off)
  const float dl = diffuse * ndv;
  const float shade = ambient + dl;
  return render_level(col.x * shade) | (render_level(col.y * shade) << 8) | (render_level(col.z * shade) << 16) | 0xff000000u;
}
#endif
