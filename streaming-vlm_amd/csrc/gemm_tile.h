// Device pieces every prefill GEMM tile kernel shares (gemm.hip, gemm_fp8.hip, gemm_wfp8.hip, gemm_wfp4.hip, gemm_mx.hip): the
// workgroup -> tile order, the [gate; up] row pairing and the epilogues.  A kernel's own part is its K loop; what surrounds it
// lives here once, so that the weight-code GEMMs' "EQUALS svlm_gemm_bf16 on the dequantised matrix" holds by construction.
// All kernels compute the product transposed (see gemm.hip): after the K loop lane (fr = lane % 16, fq = lane / 16) of wave
// (wm, wn) holds, in acc[i][j], row m = m0 + wm * 16 TM + i * 16 + fr and the four columns n = n0 + wn * 64 + j * 16 + fq * 4 + r.
#pragma once
#include "common.h"

// ---- workgroup -> (tile, K-split).  Workgroups are dealt round-robin over the 8 XCDs (private 4 MiB L2 each), so
// bid % 8 names the XCD group.  Speed only, never correctness:
//   split-K : the split index varies fastest -> an XCD only ever touches ONE K-slice of A and W (fits its L2)
//   no split: each XCD owns a contiguous range of n-tiles and walks m fastest -> a W tile is fetched once and
//             reused by all m-tiles from L2, the (smaller) A panel is what gets re-streamed
// false: a padding workgroup, which returns as a whole.
__device__ __forceinline__ bool gemm_tile_of(int bid, int gm, int gn, int splits, int& tm, int& tn, int& split) {
  if (splits > 1) {
    split = bid % splits;
    const int t = bid / splits;
    tn = t % gn;
    tm = t / gn;
  } else {
    split = 0;
    const int npx = (gn + 7) / 8;
    const int local = bid / 8;
    tn = (bid % 8) * npx + local / gm;
    tm = local % gm;
    if (tn >= gn) return false;    // whole workgroup: the grid is padded to 8 * npx * gm
  }
  return true;
}

// W row of tile row `row` (clamped: rows past N are computed on a valid row and never stored).  SwiGLU pairing: tile rows 0..63 are
// gate rows n0.., tile rows 64..127 the matching up rows N + n0.. (N = output columns)
__device__ __forceinline__ int w_row(int row, int n0, int N, bool swiglu) {
  return swiglu ? (row < 64 ? min(n0 + row, N - 1) : N + min(n0 + row - 64, N - 1)) : min(n0 + row, N - 1);
}

// plain epilogue: y = bf16(acc + bias[n]);  y = act(y);  y = bf16(y + residual[m, n]), or the raw fp32 slab of a K-split.  The
// bias / act / residual lines are written out here and once more in gemm_splitk_reduce_kernel (gemm.hip): as a helper of their own,
// nested in this one, they moved registers in every tile kernel and put the 320-row tile into scratch.
// lane holds m = fr (column of D), n = 4*fq + r (rows of D)
template <int TM>
__device__ __forceinline__ void gemm_tile_epilogue(const f32x4_t (&acc)[TM][4], int m0, int n0, int wm, int wn, int fr, int fq, int split,
                                                   int M, int N, const bf16_t* bias, const bf16_t* residual, int ldr,
                                                   bf16_t* C, int ldc, float* partial, int act) {
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wm * 16 * TM + i * 16 + fr;
    if (m >= M) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + wn * 64 + j * 16 + fq * 4;
      if (n >= N) continue;
      if (partial) {  // split-K: raw fp32 slab, the epilogue runs in the reduce kernel
        *reinterpret_cast<f32x4_t*>(partial + ((size_t)split * M + m) * N + n) = acc[i][j];
        continue;
      }
      float y[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
      if (bias) {
        u32x2_t bv = *reinterpret_cast<const u32x2_t*>(bias + n);
        y[0] += lo_bf(bv[0]); y[1] += hi_bf(bv[0]); y[2] += lo_bf(bv[1]); y[3] += hi_bf(bv[1]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) y[r] = apply_act(rbf(y[r]), act);
      if (residual) {
        u32x2_t rv = *reinterpret_cast<const u32x2_t*>(residual + (size_t)m * ldr + n);
        y[0] = y[0] + lo_bf(rv[0]); y[1] = y[1] + hi_bf(rv[0]); y[2] = y[2] + lo_bf(rv[1]); y[3] = y[3] + hi_bf(rv[1]);
      }
      u32x2_t o;
      o[0] = pack2(y[0], y[1]);
      o[1] = pack2(y[2], y[3]);
      *reinterpret_cast<u32x2_t*>(C + (size_t)m * ldc + n) = o;
    }
  }
}

// SVLM_ACT_SWIGLU (64 output columns per tile: the waves wn = 0 hold the gate half, wn = 1 the up half of the 128 tile rows of W):
// the up half (waves wn = 1) hands its bf16-rounded values to the gate half through the staging LDS, which is free now
template <int TM>
__device__ __forceinline__ void gemm_tile_epilogue_swiglu(const f32x4_t (&acc)[TM][4], unsigned char* smem, int m0, int n0, int wm, int wn,
                                                          int fr, int fq, int M, int N, const bf16_t* bias, bf16_t* C, int ldc) {
  float* U = reinterpret_cast<float*>(smem);                       // [BM][64]: BM x 256 B, below every kernel's ring of stages
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");
  if (wn == 1) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        f32x4_t u;
        const int nb = min(n0 + j * 16 + fq * 4, N - 4);
        float ub[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {                                        // up bias = second half of the [gate; up] bias vector
          const u32x2_t bv = *reinterpret_cast<const u32x2_t*>(bias + N + nb);
          ub[0] = lo_bf(bv[0]); ub[1] = hi_bf(bv[0]); ub[2] = lo_bf(bv[1]); ub[3] = hi_bf(bv[1]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) u[r] = rbf(acc[i][j][r] + ub[r]);
        *reinterpret_cast<f32x4_t*>(U + (wm * 16 * TM + i * 16 + fr) * 64 + j * 16 + fq * 4) = u;
      }
  }
  __syncthreads();
  if (wn == 0) {
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int m = m0 + wm * 16 * TM + i * 16 + fr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + fq * 4;
        if (m >= M || n >= N) continue;
        const f32x4_t u = *reinterpret_cast<const f32x4_t*>(U + (wm * 16 * TM + i * 16 + fr) * 64 + j * 16 + fq * 4);
        float h[4], gb[4] = {0.f, 0.f, 0.f, 0.f};
        if (bias) {
          const u32x2_t bv = *reinterpret_cast<const u32x2_t*>(bias + n);
          gb[0] = lo_bf(bv[0]); gb[1] = hi_bf(bv[0]); gb[2] = lo_bf(bv[1]); gb[3] = hi_bf(bv[1]);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) h[r] = apply_act(rbf(acc[i][j][r] + gb[r]), SVLM_ACT_SILU) * u[r];
        u32x2_t o;
        o[0] = pack2(h[0], h[1]);
        o[1] = pack2(h[2], h[3]);
        *reinterpret_cast<u32x2_t*>(C + (size_t)m * ldc + n) = o;
      }
    }
  }
}
