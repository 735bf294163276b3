// light_host.hip — the light kernel's own code (csrc/dev_light.h: __host__ __device__) evaluated on the CPU, behind the depth and shade
// kernels' code as tests/render_host/render_host.hip runs it (included here: depth, geom id and normal come from render_host_image).
// Built as a shared object by tests/test_light_host.py, never run on a GPU.  light_host_image() renders ONE env's width x height image
// from world-frame float32 rays, tile by tile as mjh_light_kernel does: per light the lanes that cast a shadow ray, the sphere around
// their origins (the wave reductions are loops over the tile's lanes here), the staging passes with light_cull_keep, and ray_walk.
// Lights are given in the world frame: one body at the origin carries them all.
#include "../render_host/render_host.hip"
#include "../../mujoco_sim_amd/csrc/dev_light.h"

// lights [nlight][16]: pos 3, dir 3 (unit), diffuse 3, ambient 3, cos(cutoff), exponent, directional (0 / 1), castshadow (0 / 1)
extern "C" int light_host_image(int ngeom, const float* gpos, const float* gmat, const float* gsize, const int* gtype, const int* gdata,
                                int nhf, const int* hf_dim, const float* hf_size, const int* hf_adr, const float* hf_data,
                                int nmesh, const int* plane_adr, const int* plane_num, const float* planes, const float* mesh_rbound,
                                const int* tri_adr, const int* tri_num, const double* tris, const float* color,
                                int width, int height, const float* P, const float* V, float ambient, float diffuse, const float* background,
                                int nlight, const float* lights, int shadows, int cull, float bias,
                                float* depth, int* gid, float* normal, unsigned* rgba) {
  const int nray = width * height;
  if (nlight < 0 || nlight > MJH_MAXLIGHT) return -2;
  int rc = render_host_image(ngeom, gpos, gmat, gsize, gtype, gdata, nhf, hf_dim, hf_size, hf_adr, hf_data, nmesh, plane_adr, plane_num, planes,
                             mesh_rbound, tri_adr, tri_num, tris, color, nray, P, V, 0, ambient, diffuse, background, depth, gid, normal, rgba);
  if (rc) return rc;
  // the scene again, as render_host_image builds it
  std::vector<int4> gi((size_t)ngeom);
  bool any_tri = false;
  for (int g = 0; g < ngeom; g++) { gi[g] = make_int4(gtype[g], g + 1, 0, gdata[g]); any_tri = any_tri || gtype[g] == RAY_TYPE_TRIMESH; }
  std::vector<RayHField> hf((size_t)(nhf > 0 ? nhf : 1));
  for (int h = 0; h < nhf; h++) {
    hf[h].nrow = hf_dim[2*h]; hf[h].ncol = hf_dim[2*h + 1]; hf[h].adr = hf_adr[h]; hf[h].pad = 0;
    for (int k = 0; k < 4; k++) hf[h].size[k] = hf_size[4*h + k];
  }
  std::vector<RayMesh> mesh((size_t)(nmesh > 0 ? nmesh : 1));
  std::vector<float4> pl;
  std::vector<RayTriMesh> tmesh((size_t)(nmesh > 0 ? nmesh : 1), RayTriMesh{0, 0, 0, 0, 0.0f, 0.0f, 0.0f, 0.0f});
  std::vector<RayNode> nodes; std::vector<float> trec;
  for (int i = 0; i < nmesh; i++) {
    ray_append_planes(planes + 4 * (size_t)plane_adr[i], plane_num[i], mesh_rbound[i], pl, mesh[i]);
    if (tri_num[i] > 0 && ray_append_bvh(tris + 9 * (size_t)tri_adr[i], tri_num[i], nodes, trec, tmesh[i]) != 0) return -1;
  }
  if (pl.empty()) pl.push_back(make_float4(0.0f, 0.0f, 0.0f, 1.0f));
  if (nodes.empty()) nodes.push_back(RayNode{});
  if (trec.empty()) trec.resize(RAY_TRI_FLOATS, 0.0f);
  RayScene W{};
  W.gpos = gpos; W.gmat = gmat; W.size = gsize; W.size_stride = 0; W.slot_mask = nullptr; W.sbase = 0; W.ginfo = gi.data();
  W.hf = hf.data(); W.hf_data = hf_data; W.mesh = mesh.data(); W.planes = pl.data();
  W.env0 = 0; W.n = 1; W.ngeom = ngeom; W.nbody = ngeom + 1; W.bodyexclude = -1; W.flg_static = 1; W.cutoff = 0.0f;
  RayTris T{nullptr, nullptr, nullptr};
  if (any_tri) { T.mesh = tmesh.data(); T.nodes = nodes.data(); T.tris = (const float4*)trec.data(); }
  const unsigned bg = render_pack(background[0], background[1], background[2], background[3]);
  const float bp[3] = {0.0f, 0.0f, 0.0f}, bq[4] = {1.0f, 0.0f, 0.0f, 0.0f};

  std::vector<float> recs((size_t)RAY_PASS * RAY_REC);
  const int tx = (width + DEPTH_TILE - 1) / DEPTH_TILE, ty = (height + DEPTH_TILE - 1) / DEPTH_TILE;
  for (int tile = 0; tile < tx * ty; tile++) {
    const int trow = tile / tx, tcol = tile - trow * tx;
    // the tile's live lanes
    int pix[RAY_TILE], nl = 0;
    for (int lane = 0; lane < RAY_TILE; lane++) {
      const int pi = trow * DEPTH_TILE + (lane >> 3), pj = tcol * DEPTH_TILE + (lane & 7);
      if (pi < height && pj < width) pix[nl++] = pi * width + pj;
    }
    float h[RAY_TILE][3], sum[RAY_TILE][3];
    for (int a = 0; a < nl; a++) {
      const int i = pix[a];
      for (int k = 0; k < 3; k++) { h[a][k] = P[3*i + k] + depth[i] * V[3*i + k]; sum[a][k] = 0.0f; }
    }
    for (int l = 0; l < nlight; l++) {
      const float* q = lights + 16 * l;
      LightRec R;
      R.body = 0; R.flags = (q[14] != 0.0f ? LIGHT_DIRECTIONAL : 0) | (q[15] != 0.0f ? LIGHT_CASTSHADOW : 0);
      for (int k = 0; k < 3; k++) { R.pos[k] = q[k]; R.dir[k] = q[3 + k]; R.dif[k] = q[6 + k]; R.amb[k] = q[9 + k]; }
      R.coscut = q[12]; R.exponent = q[13];
      const bool directional = (R.flags & LIGHT_DIRECTIONAL) != 0;
      float Lw[3], dw[3];
      light_frame(R, bp, bq, Lw, dw);
      float ndl[RAY_TILE], spot[RAY_TILE], ob[RAY_TILE][3], sv[RAY_TILE][3], svv[RAY_TILE], best[RAY_TILE];
      int bestg[RAY_TILE];
      bool walking[RAY_TILE], blocked[RAY_TILE], any = false;
      for (int a = 0; a < nl; a++) {
        const int i = pix[a];
        ndl[a] = light_terms(R, Lw, dw, h[a], normal + 3 * i, spot[a]);
        light_shadow_ray(R, Lw, dw, h[a], normal + 3 * i, bias, ob[a], sv[a]);
        svv[a] = sv[a][0]*sv[a][0] + sv[a][1]*sv[a][1] + sv[a][2]*sv[a][2];
        walking[a] = gid[i] >= 0 && shadows && (R.flags & LIGHT_CASTSHADOW) && ndl[a] > 0.0f && spot[a] > 0.0f && svv[a] > 0.0f && svv[a] < 3.0e38f;
        blocked[a] = false; best[a] = directional ? -1.0f : 1.0f; bestg[a] = directional ? -1 : ngeom;
        any = any || walking[a];
      }
      if (any) {
        float ct[3], rt = 0.0f, axis[3];
        for (int k = 0; k < 3; k++) {
          float lo = 3.0e38f, hi = -3.0e38f;
          for (int a = 0; a < nl; a++) if (walking[a]) { lo = fminf(lo, ob[a][k]); hi = fmaxf(hi, ob[a][k]); }
          ct[k] = 0.5f * (lo + hi);
        }
        for (int a = 0; a < nl; a++) if (walking[a]) {
          const float e[3] = {ob[a][0] - ct[0], ob[a][1] - ct[1], ob[a][2] - ct[2]};
          rt = fmaxf(rt, sqrtf(e[0]*e[0] + e[1]*e[1] + e[2]*e[2]));
        }
        rt *= 1.00001f;
        for (int k = 0; k < 3; k++) axis[k] = directional ? -dw[k] : Lw[k] - ct[k];
        for (int base = 0; base < ngeom; base += RAY_PASS) {
          int cnt = 0;
          for (int lane = 0; lane < RAY_PASS && base + lane < ngeom; lane++) {
            const int g = base + lane;
            float rb;
            const int type = any_tri ? ray_verdict<true>(W, gi[g], gsize + 3 * g, 0u, rb, &T) : ray_verdict<false>(W, gi[g], gsize + 3 * g, 0u, rb);
            if (type < 0) continue;
            if (cull && gi[g].x >= MJH_GEOM_SPHERE && !light_cull_keep(ct, rt, axis, directional, gpos + 3 * g, rb)) continue;
            ray_store(recs.data() + cnt * RAY_REC, gpos + 3 * g, gmat + 9 * g, gsize + 3 * g, rb, type, gi[g].w, g);
            cnt++;
          }
          bool left = false;
          for (int a = 0; a < nl; a++) {
            if (any_tri) ray_walk<false, true>(W, recs.data(), cnt, ob[a], sv[a], svv[a], walking[a], best[a], bestg[a], &T);
            else ray_walk<false, false>(W, recs.data(), cnt, ob[a], sv[a], svv[a], walking[a], best[a], bestg[a]);
            if (walking[a] && (directional ? bestg[a] >= 0 : best[a] < 1.0f)) { blocked[a] = true; walking[a] = false; }
            left = left || walking[a];
          }
          if (!left) break;
        }
      }
      for (int a = 0; a < nl; a++) {
        const float t = blocked[a] ? 0.0f : fmaxf(ndl[a], 0.0f) * spot[a];
        for (int k = 0; k < 3; k++) sum[a][k] += R.amb[k] + R.dif[k] * t;
      }
    }
    for (int a = 0; a < nl; a++) {
      const int i = pix[a], g = gid[i];
      const float* v = V + 3 * i;
      const float vv = v[0]*v[0] + v[1]*v[1] + v[2]*v[2];
      rgba[i] = g >= 0 ? light_color(make_float4(color[4*g], color[4*g+1], color[4*g+2], color[4*g+3]), ambient + diffuse * light_ndv(normal + 3 * i, v, vv), sum[a]) : bg;
    }
  }
  return 0;
}
