// ray_tables.h — the layout of the two per-mesh ray tables, in one place: how a mesh asset's hull planes go into RayScene::planes and
// how its BVH goes into RayTris::nodes / tris, with the asset's row of RayScene::mesh / RayTris::mesh.  Host only.  engine.hip appends
// the model's meshes with these and uploads the arrays, tests/render_host appends a scene's: the host tests walk the tables the engine
// builds.  What a caller keeps: which meshes are valid, where rbound comes from, the dummy element of an empty array, error texts.
#pragma once
#include <vector>

#include "dev_ray.h"

// mesh hull: `num` planes (n.x, n.y, n.z, d), four S each (num 0: a mesh without a hull), appended to pl and padded to a multiple of
// four with (0, 0, 0, 1), which clips nothing (dev_ray.h: ray_convex); row: the asset's RayMesh
template <class S>
inline void ray_append_planes(const S* planes, int num, float rbound, std::vector<float4>& pl, RayMesh& row) {
  row.adr = (int)pl.size(); row.rbound = rbound; row.pad = 0.0f;
  for (int k = 0; k < num; k++) pl.push_back(make_float4((float)planes[4*k], (float)planes[4*k+1], (float)planes[4*k+2], (float)planes[4*k+3]));
  while (pl.size() % 4) pl.push_back(make_float4(0.0f, 0.0f, 0.0f, 1.0f));
  row.num = (int)pl.size() - row.adr;
}

// mesh triangles: the BVH of ntri triangles (9 doubles each: ray_bvh.h) appended to the shared node and triangle-record arrays; row: the
// asset's RayTriMesh.  0, RAY_APPEND_NO_BVH (ray_bvh_build refused the triangles) or RAY_APPEND_TOO_MANY (an int offset would overflow);
// nothing is appended unless 0
enum { RAY_APPEND_NO_BVH = 1, RAY_APPEND_TOO_MANY = 2 };
inline int ray_append_bvh(const double* tri, int ntri, std::vector<RayNode>& nodes, std::vector<float>& tris, RayTriMesh& row) {
  RayBvh B;
  if (!ray_bvh_build(tri, ntri, B)) return RAY_APPEND_NO_BVH;
  if (nodes.size() + B.nodes.size() > 0x7fffffffull || tris.size() / RAY_TRI_FLOATS + (size_t)ntri > 0x0fffffffull) return RAY_APPEND_TOO_MANY;
  row = RayTriMesh{(int)nodes.size(), (int)B.nodes.size(), (int)(tris.size() / RAY_TRI_FLOATS), ntri, B.rbound, B.r1, 0.0f, 0.0f};
  nodes.insert(nodes.end(), B.nodes.begin(), B.nodes.end());
  tris.insert(tris.end(), B.tris.begin(), B.tris.end());
  return 0;
}
