// Stand-alone check of csrc/window_tiles.h: the matrix-core tile build against the broadcast multiply-add loop, bit for bit, and both
// against the k-ordered fmaf chain computed on the host.  One wavefront per case.  Exit status 0: every bit equal; 1: a difference (the first one
// is printed); 2: a HIP error.  Built and run by tests/test_gpu_window_tiles.py:
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -I mujoco_sim_amd/csrc tests/window_tiles/tiles_check.hip -o tiles_check
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "window_tiles.h"

constexpr int NK = 24, NLANE = 64, NOUT = 4;      // outputs per case: tile(A, B), and the pair's tile(A, A), tile(B, B), cross(A, B)

// in: [case][A, B][k][lane]; out: [case][NOUT][s][lane]
template <bool MFMA> __global__ __launch_bounds__(64) void tiles_kernel(const float* __restrict__ in, float* __restrict__ out) {
  const int lane = threadIdx.x;
  const float* a = in + (size_t)blockIdx.x * 2 * NK * NLANE + lane;
  float A[NK], B[NK], A2[NK], B2[NK];
#pragma unroll
  for (int k = 0; k < NK; k++) { A[k] = A2[k] = a[k * NLANE]; B[k] = B2[k] = a[(NK + k) * NLANE]; }
  float t[16], u[16], v[16], x[16];
  wn_tile16<NK, MFMA>(A, B, t);
  wn_tile16_pair<NK, MFMA>(A2, B2, u, v, x);
  float* o = out + (size_t)blockIdx.x * NOUT * 16 * NLANE + lane;
#pragma unroll
  for (int s = 0; s < 16; s++) { o[s * NLANE] = t[s]; o[(16 + s) * NLANE] = u[s]; o[(32 + s) * NLANE] = v[s]; o[(48 + s) * NLANE] = x[s]; }
}

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)

struct Case { std::string name; std::vector<float> in; };      // in: [A, B][k][lane]

static std::mt19937 rng(0x57494c45u);
static float uni(float lo, float hi) { return std::uniform_real_distribution<float>(lo, hi)(rng); }

// one hand-over row expanded the way wn_load_row does: at most two body slots of six out of NK, zeros elsewhere; a few entries exactly -0
static void expand_row(float* J /* stride NLANE */, const float scale_lo, const float scale_hi, const bool live) {
  for (int k = 0; k < NK; k++) J[k * NLANE] = 0.0f;
  if (!live) return;
  const int b1 = (int)(rng() % 4), b2 = (rng() % 4 == 0) ? -1 : (int)((b1 + 1 + rng() % 3) % 4);
  const float scale = scale_lo * std::pow(scale_hi / scale_lo, uni(0.0f, 1.0f));
  for (int b = 0; b < 4; b++) for (int j = 0; j < 6; j++) {
    float v = 0.0f;
    if (b == b1 || b == b2) { v = uni(-1.0f, 1.0f) * scale; if (rng() % 16 == 0) v = -0.0f; if (rng() % 16 == 0) v = 0.0f; }
    J[(6 * b + j) * NLANE] = v;
  }
}

// live(g, q): whether row q of lane group g is a row at all; a_same: A the same in all four groups (the 64-row form's use); sym: B = A
static Case make_case(const std::string& name, const float lo, const float hi, const bool sym, const bool a_same, bool (*live)(int, int, int), const int arg) {
  Case c{name, std::vector<float>(2 * NK * NLANE)};
  float* A = c.in.data(); float* B = A + NK * NLANE;
  for (int g = 0; g < 4; g++) for (int q = 0; q < 16; q++) {
    const int l = 16 * g + q;
    expand_row(A + l, lo, hi, live(g, q, arg));
    if (sym) for (int k = 0; k < NK; k++) B[k * NLANE + l] = A[k * NLANE + l];
    else expand_row(B + l, lo, hi, live(g, q, arg));
  }
  if (a_same) for (int l = 16; l < NLANE; l++) for (int k = 0; k < NK; k++) A[k * NLANE + l] = A[k * NLANE + (l & 15)];
  return c;
}

static uint32_t bits(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

int main() {
  std::vector<Case> cases;
  // ---- the layout case: A_(g,s) = (s + 16 g) e_0 + e_1, B_(g,q) = e_0 + 64 (q + 16 g) e_1  ->  acc[s] (lane (g, q)) = (s + 16 g) + 64 (q + 16 g), exact
  {
    Case c{"layout", std::vector<float>(2 * NK * NLANE, 0.0f)};
    float* A = c.in.data(); float* B = A + NK * NLANE;
    for (int l = 0; l < NLANE; l++) { A[l] = (float)l; A[NLANE + l] = 1.0f; B[l] = 1.0f; B[NLANE + l] = 64.0f * (float)l; }
    cases.push_back(c);
  }
  auto all = [](int, int, int) { return true; };
  auto groups = [](int g, int, int n) { return g < n; };           // lane groups n .. 3 all zero: a wavefront with fewer than four envs
  auto rows = [](int, int q, int n) { return q < n; };             // a last window with n live rows, zero padding behind them
  const float S_LO = 0.05f, S_HI = 30.0f;                          // S24's J^ = J / sqrt(M): entries of 0.05 .. 30
  for (int i = 0; i < 3; i++) cases.push_back(make_case("random sym " + std::to_string(i), S_LO, S_HI, true, false, all, 0));
  cases.push_back(make_case("subnormal sym", 3e-23f, 3e-20f, true, false, all, 0));          // products and partial sums of 1e-45 .. 1e-39
  cases.push_back(make_case("subnormal sym 2", 1e-21f, 1e-19f, true, false, all, 0));        // ... across the subnormal / normal border (1.2e-38)
  cases.push_back(make_case("subnormal cross", 3e-23f, 1e-19f, false, false, all, 0));
  cases.push_back(make_case("large sym", 1e17f, 3.7e18f, true, false, all, 0));             // products up to FLT_MAX / 24 (1.4e37), no overflow in 12 terms
  cases.push_back(make_case("large cross", 1e17f, 3.7e18f, false, false, all, 0));
  for (int n = 3; n >= 1; n--) cases.push_back(make_case(std::to_string(4 - n) + " lane groups zero", S_LO, S_HI, true, false, groups, n));
  cases.push_back(make_case("1 live row", S_LO, S_HI, true, false, rows, 1));
  cases.push_back(make_case("15 live rows", S_LO, S_HI, true, false, rows, 15));
  for (int i = 0; i < 2; i++) cases.push_back(make_case("cross " + std::to_string(i), S_LO, S_HI, false, false, all, 0));
  cases.push_back(make_case("64-row use", S_LO, S_HI, false, true, all, 0));
  cases.push_back(make_case("64-row use, 15 live rows", S_LO, S_HI, false, true, rows, 15));

  const int nc = (int)cases.size();
  const size_t nin = (size_t)nc * 2 * NK * NLANE, nout = (size_t)nc * NOUT * 16 * NLANE;
  std::vector<float> hin(nin), mfma(nout), valu(nout), host(nout);
  for (int c = 0; c < nc; c++) std::memcpy(hin.data() + (size_t)c * 2 * NK * NLANE, cases[c].in.data(), 2 * NK * NLANE * sizeof(float));
  float *din = nullptr, *dm = nullptr, *dv = nullptr;
  HIP_OK(hipMalloc(&din, nin * sizeof(float))); HIP_OK(hipMalloc(&dm, nout * sizeof(float))); HIP_OK(hipMalloc(&dv, nout * sizeof(float)));
  HIP_OK(hipMemcpy(din, hin.data(), nin * sizeof(float), hipMemcpyHostToDevice));
  HIP_OK(hipMemset(dm, 0xff, nout * sizeof(float))); HIP_OK(hipMemset(dv, 0xff, nout * sizeof(float)));
  tiles_kernel<true><<<nc, NLANE>>>(din, dm);
  HIP_OK(hipGetLastError());
  tiles_kernel<false><<<nc, NLANE>>>(din, dv);
  HIP_OK(hipGetLastError());
  HIP_OK(hipDeviceSynchronize());
  HIP_OK(hipMemcpy(mfma.data(), dm, nout * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipMemcpy(valu.data(), dv, nout * sizeof(float), hipMemcpyDeviceToHost));
  HIP_OK(hipFree(din)); HIP_OK(hipFree(dm)); HIP_OK(hipFree(dv));

  // the host's chain: acc = fmaf(A_(g,s)[k], B_(g,q)[k], acc), k = 0 .. NK - 1, from +0
  for (int c = 0; c < nc; c++) {
    const float* A = hin.data() + (size_t)c * 2 * NK * NLANE; const float* B = A + NK * NLANE;
    for (int o = 0; o < NOUT; o++) {
      const float* X = (o == 2) ? B : A; const float* Y = (o == 1) ? A : B;
      for (int l = 0; l < NLANE; l++) for (int s = 0; s < 16; s++) {
        float acc = 0.0f;
        for (int k = 0; k < NK; k++) acc = std::fmaf(X[k * NLANE + (l & 48) + s], Y[k * NLANE + l], acc);
        host[((size_t)(c * NOUT + o) * 16 + s) * NLANE + l] = acc;
      }
    }
  }

  static const char* const OUT_NAME[NOUT] = {"tile(A, B)", "pair: tile(A, A)", "pair: tile(B, B)", "pair: cross(A, B)"};
  int status = 0;
  size_t nsub = 0, nnegz = 0;
  auto compare = [&](const char* what, const std::vector<float>& x, const char* xn, const std::vector<float>& y, const char* yn) {
    size_t ndiff = 0;
    for (int c = 0; c < nc; c++) for (int o = 0; o < NOUT; o++) for (int l = 0; l < NLANE; l++) for (int s = 0; s < 16; s++) {
      const size_t i = ((size_t)(c * NOUT + o) * 16 + s) * NLANE + l;
      if (bits(x[i]) == bits(y[i])) continue;
      if (ndiff++ == 0) {
        std::printf("DIFF %s: case '%s', %s, env %d, q %d, r %d: %s %08x (%g), %s %08x (%g)\n", what, cases[c].name.c_str(), OUT_NAME[o], l >> 4, l & 15, s,
                    xn, bits(x[i]), (double)x[i], yn, bits(y[i]), (double)y[i]);
        if (c == 0) {      // the layout case: say whose value arrived
          const int v = (int)x[i];
          std::printf("  layout: lane (%d, %d) register %d holds the entry of lane (%d, %d) register %d\n", l >> 4, l & 15, s, (v / 64) >> 4, (v / 64) & 15, (v % 64) & 15);
        }
      }
    }
    std::printf("%s: %zu of %zu values differ\n", what, ndiff, nout);
    if (ndiff) status = 1;
  };
  compare("matrix cores vs broadcast multiply-adds", mfma, "mfma", valu, "bcast");
  compare("matrix cores vs host fmaf chain", mfma, "mfma", host, "host");
  compare("broadcast multiply-adds vs host fmaf chain", valu, "bcast", host, "host");
  for (size_t i = 0; i < nout; i++) { const uint32_t b = bits(host[i]); nsub += ((b & 0x7f800000u) == 0 && (b & 0x007fffffu) != 0); nnegz += b == 0x80000000u; }
  std::printf("cases %d, values %zu, subnormal results %zu, -0 results %zu\n", nc, nout, nsub, nnegz);
  std::printf(status ? "FAILED\n" : "IDENTICAL\n");
  return status;
}
