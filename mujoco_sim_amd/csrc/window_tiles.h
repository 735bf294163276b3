// Tile rows of the window forms (window_kernel.h): sixteen k-ordered dot products per lane, built on the matrix cores.
//
// A wavefront is four 16-lane groups g (one env each in the 16-row form), lane (g, q) = 16 g + q.  Given one float per lane and dof slot k,
//   acc[s] (lane (g, q)) = sum_k A_(g,s)[k] * B_(g,q)[k],       s = 0 .. 15,
// summed in k order from +0 with one fused multiply-add per k: acc = fma(A_(g,s)[k], B_(g,q)[k], acc).
//
// WN_TILE_MFMA = 1: v_mfma_f32_16x16x1_4b_f32, one per k on ONE 16-register accumulator.  Its four blocks are four independent 16 x 16
// outer-product steps, block b reading its A and B entries from lanes 16 b .. 16 b + 15 — the layout the J^ registers already have.  An f32
// MFMA step is one fused multiply-add per entry (one rounding, subnormals kept: the C/D side of an MFMA never flushes, A/B follow the
// kernel's denormal mode), so 24 dependent steps are the same chain as 24 broadcast multiply-adds per entry — tests/test_gpu_window_tiles.py
// compares the two bit for bit.  The result D has register 4 b + c of lane (h, j) = D_b[4 h + c][j] = A_(b, 4 h + c) . B_(b, j): the
// sixteen columns of env b sit in registers 4 b .. 4 b + 3 of all four lane groups and come home to lane group b, register 4 h + c, by a
// 4 x 4 transpose between lane groups and register quads: eight v_permlane32_swap (the 2 x 2 blocks), then eight v_permlane16_swap.
// WN_TILE_MFMA = 0: the broadcast multiply-add loop (v_fmac_f32_dpp row_newbcast, 16 per k) under the same signature.
#pragma once

#ifndef WN_TILE_MFMA
#define WN_TILE_MFMA 1
#endif

#ifndef WN_TILE_CHAINS
#define WN_TILE_CHAINS 3      // independent accumulator chains of a window pair's three tiles (3: 48 registers; 1: one after the other)
#endif

typedef float wn_f32x16 __attribute__((ext_vector_type(16)));

// ---- the matrix-core form
template <int NK> __device__ __forceinline__ wn_f32x16 wn_tile16_mma(const float* A, const float* B) {
  wn_f32x16 d = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < NK; k++) d = __builtin_amdgcn_mfma_f32_16x16x1f32(A[k], B[k], d, 0, 0, 0);
  return d;
}

// D (register 4 b + c of lane group h: block b, rows 4 h + c) -> acc (register 4 h + c of lane group b)
__device__ __forceinline__ void wn_tile16_home(const wn_f32x16 d, float* acc) {
  unsigned r[16];
#pragma unroll
  for (int i = 0; i < 16; i++) { const float x = d[i]; r[i] = __builtin_bit_cast(unsigned, x); }       // (through a float: a bit cast of the vector's element itself reads element 0)
  // the 2 x 2 blocks: lane groups 2, 3 of register quads 0, 1 <-> lane groups 0, 1 of register quads 2, 3
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const auto p = __builtin_amdgcn_permlane32_swap(r[i], r[i + 8], false, false);
    r[i] = p[0]; r[i + 8] = p[1];
  }
  // inside each block: the odd lane group of the even register quad <-> the even lane group of the odd quad
#pragma unroll
  for (int i = 0; i < 16; i++) if (!(i & 4)) {
    const auto p = __builtin_amdgcn_permlane16_swap(r[i], r[i + 4], false, false);
    r[i] = p[0]; r[i + 4] = p[1];
  }
#pragma unroll
  for (int i = 0; i < 16; i++) acc[i] = __builtin_bit_cast(float, r[i]);
}

// ---- the broadcast multiply-add form (dof k outermost: consecutive multiply-adds go to different accumulators)
#define WN_TILE_FMAC_BC(acc, x, y, R) asm volatile("v_fmac_f32_dpp %0, %1, %2 row_newbcast:" #R " row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(x), "v"(y))
#define WN_TILE_BC16(M) M(0) M(1) M(2) M(3) M(4) M(5) M(6) M(7) M(8) M(9) M(10) M(11) M(12) M(13) M(14) M(15)
template <int NK> __device__ __forceinline__ void wn_tile16_bcast(float* A, float* B, float* acc) {
#pragma unroll
  for (int s = 0; s < 16; s++) acc[s] = 0.0f;
#pragma unroll
  for (int k = 0; k < NK; k++) asm volatile("" : "+v"(A[k]));     // (materialised before the DPP reads below: no VALU write within two instructions of them)
  if (A != B) {
#pragma unroll
    for (int k = 0; k < NK; k++) asm volatile("" : "+v"(B[k]));
  }
  asm volatile("s_nop 1");
#define WN_TILE_ACC(s) WN_TILE_FMAC_BC(acc[s], A[k], B[k], s);
#pragma unroll
  for (int k = 0; k < NK; k++) { WN_TILE_BC16(WN_TILE_ACC) }
#undef WN_TILE_ACC
}

// ---- one tile; A and B may be the same array (the symmetric tile)
template <int NK, bool MFMA = (WN_TILE_MFMA != 0)> __device__ __forceinline__ void wn_tile16(float* A, float* B, float* acc) {
  if constexpr (MFMA) wn_tile16_home(wn_tile16_mma<NK>(A, B), acc);
  else wn_tile16_bcast<NK>(A, B, acc);
}

// ---- the three tiles of a window pair (tile of U, tile of V, cross: lane q ends with J^_(V,q) . J^_(U,r)) as three interleaved chains:
// a dependent MFMA waits for its accumulator, three independent ones keep the matrix core issuing
template <int NK, bool MFMA = (WN_TILE_MFMA != 0)> __device__ __forceinline__ void wn_tile16_pair(float* U, float* V, float* accU, float* accV, float* accX) {
  if constexpr (MFMA && WN_TILE_CHAINS == 1) {
    wn_tile16<NK, true>(U, U, accU); __builtin_amdgcn_sched_barrier(0);
    wn_tile16<NK, true>(V, V, accV); __builtin_amdgcn_sched_barrier(0);
    wn_tile16<NK, true>(U, V, accX);
  } else if constexpr (MFMA) {
    wn_f32x16 du, dv, dx;
#pragma unroll
    for (int i = 0; i < 16; i++) { du[i] = 0.0f; dv[i] = 0.0f; dx[i] = 0.0f; }
#pragma unroll
    for (int k = 0; k < NK; k++) {
      du = __builtin_amdgcn_mfma_f32_16x16x1f32(U[k], U[k], du, 0, 0, 0);
      dv = __builtin_amdgcn_mfma_f32_16x16x1f32(V[k], V[k], dv, 0, 0, 0);
      dx = __builtin_amdgcn_mfma_f32_16x16x1f32(U[k], V[k], dx, 0, 0, 0);
    }
    wn_tile16_home(du, accU); wn_tile16_home(dv, accV); wn_tile16_home(dx, accX);
  } else {
    wn_tile16_bcast<NK>(U, U, accU); wn_tile16_bcast<NK>(V, V, accV); wn_tile16_bcast<NK>(U, V, accX);
  }
}
