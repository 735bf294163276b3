// ray_bvh.h — the tables behind a ray's view of a mesh's own triangles (mjh_ray_set_mesh_surface: MJH_RAY_SURFACE_TRIANGLES): the node
// and triangle records the device walks (dev_ray.h: ray_trimesh) and the host code that builds them per mesh asset.  Plain C++, no HIP:
// engine.hip builds and uploads the tables, tests/ray_host includes this very file.
//
// Threaded BVH.  The nodes of a mesh are stored in depth-first preorder: the left child of node i is node i + 1, and `skip` is the
// index of the first node behind i's subtree (the node count for the root).  A traversal is therefore one forward scan, i -> i + 1 (go
// down / visit) or i -> skip (the subtree is pruned), with i < skip <= n for every node: it needs no stack and ends after at most n
// steps whatever the data.  Built deterministically: split at the median of the triangle centroids along the longest axis of the
// centroid bounds, ties by triangle index, leaves of at most RAY_BVH_LEAF triangles; a leaf's triangles are contiguous in leaf order.
//
// Slack (all in units of 2^-21 = 4.8e-7, four fp32 ulps, as the height-field walk of dev_ray.h uses).  ray_tri accepts a hit only if
// the hit point p + x v, evaluated in fp32, lies in the triangle's own box widened by s' = 2^-21 (|p|_1 + R1) per axis, R1 the largest
// 1-norm of a corner of the mesh: the part 2^-21 R1 is stored in the triangle's box here, the part 2^-21 |p|_1 is the ray's own (its
// rounding grows with the distance of the origin, not with the mesh).  A node's box is that of its triangles' corners widened by
// three times as much: 3 * 2^-21 R1 stored here, 3 * 2^-21 |p|_1 added by the ray.  Why that suffices for "pruning never changes a
// result": let x be an accepted parameter and X = fl(p + x v) the point the test looked at; the exact point differs from X by at most
// one ulp of L = |p|_1 + R1 per axis (1.2e-7 L), so it lies within s' + 1.2e-7 L of the triangle's box and hence of every enclosing
// node's corner box.  The slab test computes (b -+ sn - p) * (1 / v_k) with sn = 3 s': one rounding of p +- sn (0.6e-7 L), one of the
// difference (0.6e-7 L) and two relative ones (1.2e-7 of a value below L / |v_k|), together under 3.6e-7 L / |v_k| in the parameter,
// while the exact entry into the widened box precedes x by at least (sn - s' - 1.2e-7 L) / |v_k| = 8.3e-7 L / |v_k|.  So the computed
// entry of every ancestor box is <= x and the computed exit >= x: the box is hit, and "entry <= best so far" can only prune
// triangles whose x is above the best.  Boxes are rounded outwards to float32 before the margin is added.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#define RAY_BVH_LEAF 4              // triangles per leaf at most
#define RAY_TRI_FLOATS 16           // floats of a triangle record (four float4)
#define RAY_SLACK 4.76837158e-7f    // 2^-21
#define RAY_NODE_SLACK 3.0f         // a node's box is widened by this many RAY_SLACK (see above)

// 32 bytes, 32-byte aligned in the table: one s_load_dwordx8.  leaf < 0: inner node; else (first triangle << 3) | count, the first
// triangle counted from the mesh's first
struct RayNode { float bmin[3], bmax[3]; int skip, leaf; };
static_assert(sizeof(RayNode) == 32, "RayNode is one 32-byte record");

// a mesh asset's rows of the tables: nodes [node, node + nnode), triangle records from `tri` on (in triangles); rbound: the largest
// |corner| of its triangles (the bounding sphere of the walk: NOT the hull table's, the kept vertices are an inner approximation);
// r1: the largest 1-norm of a corner
struct RayTriMesh { int node, nnode, tri, ntri; float rbound, r1, pad0, pad1; };

// triangle record, 64 bytes: (a.xyz, |e1|_1) (e1.xyz, lo.x) (e2.xyz, lo.y) (lo.z, hi.x, hi.y, hi.z) with e1 = b - a, e2 = c - a and
// [lo, hi] the triangle's box widened by RAY_SLACK * r1
struct RayBvh {
  std::vector<RayNode> nodes;
  std::vector<float> tris;      // RAY_TRI_FLOATS per triangle, in leaf order
  std::vector<int> order;       // order[k]: the input triangle stored as record k
  float rbound = 0.0f, r1 = 0.0f;
};

inline float ray_bvh_down(double d) { float f = (float)d; return (double)f > d ? std::nextafterf(f, -INFINITY) : f; }
inline float ray_bvh_up(double d) { float f = (float)d; return (double)f < d ? std::nextafterf(f, INFINITY) : f; }

namespace ray_bvh_detail {
struct Builder {
  const double* tri; RayBvh& out; std::vector<int> idx; std::vector<double> cen; double pad_node, pad_tri;
  void bounds(int lo, int hi, double* mn, double* mx) const {
    for (int k = 0; k < 3; k++) { mn[k] = 1e300; mx[k] = -1e300; }
    for (int i = lo; i < hi; i++) for (int c = 0; c < 3; c++) for (int k = 0; k < 3; k++) {
      const double x = tri[9 * (size_t)idx[i] + 3 * c + k];
      mn[k] = std::min(mn[k], x); mx[k] = std::max(mx[k], x);
    }
  }
  void build(int lo, int hi) {
    const int i = (int)out.nodes.size();
    out.nodes.push_back(RayNode{});
    double mn[3], mx[3];
    bounds(lo, hi, mn, mx);
    for (int k = 0; k < 3; k++) { out.nodes[i].bmin[k] = ray_bvh_down((double)ray_bvh_down(mn[k]) - pad_node); out.nodes[i].bmax[k] = ray_bvh_up((double)ray_bvh_up(mx[k]) + pad_node); }
    if (hi - lo <= RAY_BVH_LEAF) {
      out.nodes[i].leaf = ((int)out.order.size() << 3) | (hi - lo);
      for (int j = lo; j < hi; j++) out.order.push_back(idx[j]);
      out.nodes[i].skip = i + 1;
      return;
    }
    double cmn[3] = {1e300, 1e300, 1e300}, cmx[3] = {-1e300, -1e300, -1e300};
    for (int j = lo; j < hi; j++) for (int k = 0; k < 3; k++) { cmn[k] = std::min(cmn[k], cen[3 * (size_t)idx[j] + k]); cmx[k] = std::max(cmx[k], cen[3 * (size_t)idx[j] + k]); }
    int ax = 0;
    for (int k = 1; k < 3; k++) if (cmx[k] - cmn[k] > cmx[ax] - cmn[ax]) ax = k;
    std::sort(idx.begin() + lo, idx.begin() + hi, [&](int a, int b) { const double ca = cen[3 * (size_t)a + ax], cb = cen[3 * (size_t)b + ax]; return ca < cb || (ca == cb && a < b); });
    const int mid = lo + (hi - lo) / 2;
    build(lo, mid);
    build(mid, hi);
    out.nodes[i].leaf = -1;
    out.nodes[i].skip = (int)out.nodes.size();
  }
};
}  // namespace ray_bvh_detail

// the invariants a traversal relies on: i < skip <= n for every node, i + 1 == skip and 1 .. RAY_BVH_LEAF triangles inside [0, ntri) for a leaf
inline bool ray_bvh_check(const RayBvh& B) {
  const int n = (int)B.nodes.size(), nt = (int)B.order.size();
  if (n <= 0 || B.nodes[0].skip != n || B.tris.size() != (size_t)RAY_TRI_FLOATS * (size_t)nt) return false;
  for (int i = 0; i < n; i++) {
    const RayNode& N = B.nodes[i];
    if (!(i < N.skip && N.skip <= n)) return false;
    if (N.leaf >= 0) {
      const int first = N.leaf >> 3, cnt = N.leaf & 7;
      if (N.skip != i + 1 || cnt < 1 || cnt > RAY_BVH_LEAF || first < 0 || first + cnt > nt) return false;
    }
  }
  return true;
}

// tri: ntri triangles as 9 doubles each (a, b, c) in the mesh's frame, ntri >= 1 and below 2^28.  false: bad input or a violated invariant
inline bool ray_bvh_build(const double* tri, int ntri, RayBvh& out) {
  out = RayBvh{};
  if (!tri || ntri < 1 || ntri >= (1 << 28)) return false;
  double r2 = 0, r1 = 0;
  for (size_t i = 0; i < 3 * (size_t)ntri; i++) {
    const double* x = tri + 3 * i;
    if (!(std::isfinite(x[0]) && std::isfinite(x[1]) && std::isfinite(x[2]))) return false;
    r2 = std::max(r2, x[0]*x[0] + x[1]*x[1] + x[2]*x[2]); r1 = std::max(r1, std::fabs(x[0]) + std::fabs(x[1]) + std::fabs(x[2]));
  }
  out.rbound = ray_bvh_up(std::sqrt(r2)); out.r1 = ray_bvh_up(r1);
  ray_bvh_detail::Builder b{tri, out, std::vector<int>((size_t)ntri), std::vector<double>(3 * (size_t)ntri), (double)RAY_NODE_SLACK * (double)RAY_SLACK * (double)out.r1, (double)RAY_SLACK * (double)out.r1};
  for (int i = 0; i < ntri; i++) {
    b.idx[i] = i;
    for (int k = 0; k < 3; k++) b.cen[3 * (size_t)i + k] = (tri[9 * (size_t)i + k] + tri[9 * (size_t)i + 3 + k] + tri[9 * (size_t)i + 6 + k]) / 3.0;
  }
  out.nodes.reserve(2 * (size_t)ntri); out.order.reserve((size_t)ntri);
  b.build(0, ntri);
  out.tris.resize((size_t)RAY_TRI_FLOATS * (size_t)ntri);
  for (int k = 0; k < ntri; k++) {
    const double* t = tri + 9 * (size_t)out.order[k];
    float* q = out.tris.data() + (size_t)RAY_TRI_FLOATS * (size_t)k;
    float lo[3], hi[3];
    for (int j = 0; j < 3; j++) {
      q[j] = (float)t[j]; q[4 + j] = (float)(t[3 + j] - t[j]); q[8 + j] = (float)(t[6 + j] - t[j]);
      lo[j] = ray_bvh_down((double)ray_bvh_down(std::min(t[j], std::min(t[3 + j], t[6 + j]))) - b.pad_tri);
      hi[j] = ray_bvh_up((double)ray_bvh_up(std::max(t[j], std::max(t[3 + j], t[6 + j]))) + b.pad_tri);
    }
    q[3] = std::fabs(q[4]) + std::fabs(q[5]) + std::fabs(q[6]);
    q[7] = lo[0]; q[11] = lo[1]; q[12] = lo[2]; q[13] = hi[0]; q[14] = hi[1]; q[15] = hi[2];
  }
  return ray_bvh_check(out);
}
