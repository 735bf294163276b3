// depth_host.hip — csrc/dev_depth.h (__host__ __device__) built for the CPU: the pixel directions and the tile cull of the depth kernel,
// called by tests/test_depth_host.py through ctypes.
#include "../../mujoco_sim_amd/csrc/dev_depth.h"

extern "C" {

// out [height][width][3]
void depth_host_dirs(int width, int height, float scale, float* out) {
  for (int i = 0; i < height; i++)
    for (int j = 0; j < width; j++) depth_pixel_dir(i, j, width, height, scale, out + 3 * ((size_t)i * width + j));
}

// tile (trow, tcol) of every case against its sphere (centre relative to the camera origin, camera frame): keep[k] = the predicate's verdict
void depth_host_cull(int width, int height, float scale, int ncase, const int* trow, const int* tcol, const float* centre, const float* radius, int* keep) {
  for (int k = 0; k < ncase; k++) {
    const int i0 = trow[k] * DEPTH_TILE, j0 = tcol[k] * DEPTH_TILE;
    const int ni = height - i0 < DEPTH_TILE ? height - i0 : DEPTH_TILE, nj = width - j0 < DEPTH_TILE ? width - j0 : DEPTH_TILE;
    float axis[3], cosA, sinA;
    depth_tile_cone(i0, j0, ni, nj, width, height, scale, axis, cosA, sinA);
    keep[k] = depth_cone_keep(axis, cosA, sinA, centre + 3 * k, radius[k]) ? 1 : 0;
  }
}

}
