// Weight-fp8, activation-bf16 MFMA GEMM:  C[M,N] = epi(A[M,K] . W'[N,K]^T),  W'[n,k] = e4m3(W8[n,k]) * w_scale[n]
//   epi: the tile epilogues of gemm_tile.h (bias, activations 0..3, residual incl. in place, SVLM_ACT_SWIGLU on [gate rows; up rows],
//   split-K through the caller's workspace, the norm of the output row inside the split-K reduce); plan and launch: gemm_plan.h.
// The prefill of an `llm_fp8` engine reads the e4m3 language-model weights with it instead of rebuilding every layer in bf16
// (svlm_dequant_fp8_bf16 + svlm_gemm_bf16): the weight tile is staged as CODES, half the bytes and half the LDS-DMA pieces per
// K-tile of gemm_glds_kernel (gemm.hip), and turned into bf16 when a wave reads its MFMA fragment -- once per W fragment, reused by
// all TM A fragments.  The row scale is a power of two (weights.py:quantize_rows_fp8_pow2) and is applied inside the conversion, so
// code * scale is exact in bf16 and the MFMA sees bit for bit the operands the scratch path feeds it: with the same K per split the
// result EQUALS svlm_gemm_bf16 on the dequantised matrix (v_mfma_f32_16x16x32_bf16, same K order, same epilogue).
//
// Replaces (prefill rows of an fp8 language model): qwen2/language_forward.py:80-82,161 and Qwen2MLP (:201).
//
// Tile (16 TM WM) x 128 x 64, 2 WM waves as WM (m) x 2 (n).  LDS stage = A tile (BM rows x 128 B, the image of gemm_glds_kernel) +
// W tile (128 rows x 64 B of codes).  A W row holds four 16-B chunks; chunk c of row r lives at position c ^ ((r >> 2) & 3): a
// fragment read is 8 B per lane (ds_read_b64, conflict groups = the two 32-lane halves, 64 banks of 4 B), a half covers 16 rows x
// 16 B, rows r, r+4, r+8, r+12 share their 16 banks and land in four different chunk positions -> conflict-free.  The DMA image is
// lane-linear (1 KiB piece = 16 rows x 64 B, lane i -> row i / 4, position i % 4), so the swizzle sits on the per-lane SOURCE
// address and again on the fragment read.
#include "common.h"
#include "gemm_plan.h"
#include "gemm_tile.h"
#include <stdlib.h>

#define WF_BN 128
#define WF_BK 64

extern __shared__ __attribute__((aligned(16))) unsigned char wfp8_dyn_smem[];

#define WF_GLDS(gp, lp) \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp), (__attribute__((address_space(3))) void*)(lp), 16, 0, 0)

// 8 e4m3 codes (k ascending from byte 0 of c[0]) times a power-of-two scale -> 8 bf16, the MFMA fragment.  v_cvt_pk_f32_fp8 is exact,
// the product with 2^e is exact in fp32 and (3 mantissa bits, exponent far inside the bf16 range) in bf16, so the rounding of the pack
// never acts: every finite code gives dequantize_rows_fp8's value (tests/test_gemm_wfp8_gpu.py: all 254 codes under four scales).
__device__ __forceinline__ bf16x8_t wfp8_fragment(const u32x2_t c, const float scale) {
  typedef float f32x2_t __attribute__((ext_vector_type(2)));
  u32x4_t o;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[h], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c[h], true);
    o[2 * h] = pack2(lo[0] * scale, lo[1] * scale);
    o[2 * h + 1] = pack2(hi[0] * scale, hi[1] * scale);
  }
  return __builtin_bit_cast(bf16x8_t, o);
}

template <int TM, int WM = 2>
__global__ __launch_bounds__(128 * WM) void gemm_wfp8_kernel(const bf16_t* __restrict__ A, int lda,
                                                             const unsigned char* __restrict__ W8, int ldw,
                                                             const float* __restrict__ w_scale,
                                                             const bf16_t* __restrict__ bias,
                                                             const bf16_t* residual, int ldr,
                                                             bf16_t* C, int ldc, float* __restrict__ partial,
                                                             int M, int N, int K, int k_per_split, int act, int gm, int gn, int splits) {
  constexpr int BM = 16 * TM * WM;
  constexpr int A_INST = TM;                    // 1-KiB DMA pieces per wave per tile: A (8 rows x 128 B each, BM / 8 pieces over 2 WM waves)
  constexpr int W_INST = 4 / WM;                // ... and W (16 rows x 64 B of codes each, 8 pieces)
  constexpr int NPT = A_INST + W_INST;          // DMA instructions per wave per tile
  constexpr int STAGE_B = BM * 128 + WF_BN * 64;
  unsigned char* smem = wfp8_dyn_smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn, split;
  if (!gemm_tile_of(blockIdx.x, gm, gn, splits, tm, tn, split)) return;
  const bool swiglu = act == SVLM_ACT_SWIGLU;     // 64 output columns per tile: gate | up halves of the 128 tile rows of W
  const int m0 = tm * BM, n0 = tn * (swiglu ? WF_BN / 2 : WF_BN);
  const int k_begin = split * k_per_split;
  const int k_end = min(K, k_begin + k_per_split);
  const int nk = (k_end - k_begin) / WF_BK;      // K % 64 == 0 and k_per_split % 64 == 0


  const bf16_t* a_src[A_INST];
  const unsigned char* w_src[W_INST];
#pragma unroll
  for (int i = 0; i < A_INST; ++i) {             // A piece: row = piece * 8 + lane / 8, position lane % 8 holds chunk p ^ (row & 7)
    const int row = (wave * A_INST + i) * 8 + (lane >> 3);
    a_src[i] = A + (size_t)min(m0 + row, M - 1) * lda + k_begin + (((lane & 7) ^ (row & 7)) * 8);
  }
#pragma unroll
  for (int i = 0; i < W_INST; ++i) {             // W piece: row = piece * 16 + lane / 4, position lane % 4 holds chunk p ^ ((row >> 2) & 3)
    const int row = (wave * W_INST + i) * 16 + (lane >> 2);
    w_src[i] = W8 + (size_t)w_row(row, n0, N, swiglu) * ldw + k_begin + (((lane & 3) ^ ((row >> 2) & 3)) * 16);
  }
  const int fr = lane & 15, fq = lane >> 4;
  // the scales of this lane's four W fragment rows; pinned here so that their loads are complete before the DMA ring starts and the
  // hand-counted vmcnt waits below see DMA pieces only
  float sc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) sc[j] = w_scale[w_row(wn * 64 + j * 16 + fr, n0, N, swiglu)];
#pragma unroll
  for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(sc[j]));

  auto issue = [&](int kt, int stage) {
    unsigned char* sa = smem + stage * STAGE_B;
    unsigned char* sw = sa + BM * 128;
#pragma unroll
    for (int i = 0; i < A_INST; ++i) WF_GLDS(a_src[i] + kt * WF_BK, sa + (wave * A_INST + i) * 1024);
#pragma unroll
    for (int i = 0; i < W_INST; ++i) WF_GLDS(w_src[i] + kt * WF_BK, sw + (wave * W_INST + i) * 1024);
  };

  f32x4_t acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // byte offsets of this lane's W fragments inside a stage's W tile: codes k = ks * 32 + fq * 8 .. + 7 = chunk ks * 2 + fq / 2, its half
  // fq & 1.  Each offset is made opaque so that the reads stay eight ds_read_b64: with a common base hipcc pairs them into
  // ds_read2st64_b64, which moves a quarter of the bytes per LDS cycle (32-bank mode).
  unsigned woff[2][4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      woff[ks][j] = (wn * 64 + j * 16 + fr) * 64 + (((ks * 2 + (fq >> 1)) ^ ((fr >> 2) & 3)) * 16) + (fq & 1) * 8;
      asm volatile("" : "+v"(woff[ks][j]));
    }
  auto compute = [&](int stage) {
    const unsigned char* sa = smem + stage * STAGE_B;
    const unsigned char* sw = sa + BM * 128;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[TM], wf[4];
      const int pos = ((ks * 4 + fq) ^ (fr & 7)) * 16;      // rows of a fragment differ by multiples of 16 -> row & 7 == fr & 7
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(sa + (wm * 16 * TM + i * 16 + fr) * 128 + pos);
#pragma unroll
      for (int j = 0; j < 4; ++j) wf[j] = wfp8_fragment(*reinterpret_cast<const u32x2_t*>(sw + woff[ks][j]), sc[j]);
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };

  // 3-stage ring, 2 tiles in flight; waits counted by hand (vmcnt(NPT) leaves the newer tile's pieces in flight), raw barrier
  constexpr int NS = 3, AHEAD = NS - 1;
#pragma unroll
  for (int t = 0; t < AHEAD; ++t)
    if (t < nk) issue(t, t);
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NPT) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    if (kt + AHEAD < nk) issue(kt + AHEAD, (kt + AHEAD) % NS);
    compute(kt % NS);
  }

  if (swiglu) {
    gemm_tile_epilogue_swiglu<TM>(acc, smem, m0, n0, wm, wn, fr, fq, M, N, bias, C, ldc);
    return;
  }
  gemm_tile_epilogue<TM>(acc, m0, n0, wm, wn, fr, fq, split, M, N, bias, residual, ldr, C, ldc, partial, act);
}

static int gemm_wfp8_impl(const void* A, int lda, const void* W8, int ldw, const float* w_scale, const void* bias, const void* residual, int ldr,
                          void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes, void* stream,
                          const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn) {
  SVLM_CHECK_ARG(M >= 0 && N > 0 && K > 0, "svlm_gemm_wfp8: bad shape M=%d N=%d K=%d", M, N, K);
  SVLM_CHECK_ARG(K % WF_BK == 0 && N % 4 == 0, "svlm_gemm_wfp8: K=%d must be a multiple of 64 and N=%d of 4", K, N);
  SVLM_CHECK_ARG(W8 != nullptr && w_scale != nullptr && ((uintptr_t)W8 & 15) == 0, "svlm_gemm_wfp8: needs 16-B aligned codes and one scale per row");
  SVLM_CHECK_ARG(lda % 8 == 0 && ldw % 16 == 0 && ldc % 4 == 0 && (!residual || ldr % 4 == 0),
                 "svlm_gemm_wfp8: leading dims must keep 16-B row alignment (lda=%d ldw=%d bytes ldc=%d ldr=%d)", lda, ldw, ldc, ldr);
  SVLM_CHECK_ARG(lda >= K && ldw >= K && ldc >= N, "svlm_gemm_wfp8: leading dim smaller than row length");
  SVLM_CHECK_ARG(act >= 0 && act <= 4, "svlm_gemm_wfp8: unknown activation %d", act);
  const bool swiglu = act == SVLM_ACT_SWIGLU;
  SVLM_CHECK_ARG(!swiglu || (residual == nullptr && norm_w == nullptr && N % 8 == 0),
                 "svlm_gemm_wfp8: SVLM_ACT_SWIGLU takes W8 = [gate; up] (scales and bias = [gate; up] too) without residual or norm, N %% 8 == 0 (N=%d)", N);
  if (M == 0) return SVLM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int gn = swiglu ? (N + WF_BN / 2 - 1) / (WF_BN / 2) : (N + WF_BN - 1) / WF_BN;
  // ---- tile height and K-split: the plan of svlm_gemm_bf16 on this kernel's tiles (gemm_plan.h:gemm_wcode_plan; a shape gets the K
  // per split its bf16 twin gets and reproduces it bit for bit), which also writes the plan note
  const GemmWPlan p = gemm_wcode_plan("SVLM_GEMM_WFP8", 2, M, N, K, gn, swiglu, ws, ws_bytes);
  float* partial = p.splits > 1 ? (float*)ws : nullptr;
  // LDS: three stages of A tile (BM rows x 128 B) + W tile of codes
#define W_LAUNCH(TM, WM)                                                                                                                   \
  gemm_launch<&gemm_wfp8_kernel<TM, WM>, 128 * WM, 3 * (16 * TM * WM * 128 + WF_BN * 64)>("svlm_gemm_wfp8", p.nblocks, st, A, lda, W8, ldw, w_scale, bias, residual, \
                                                                                  ldr, C, ldc, partial, M, N, K, p.kps, act, p.gm, gn, p.splits)
  const int rc = p.bm == 256 ? W_LAUNCH(4, 4) : p.bm == 128 ? W_LAUNCH(4, 2) : W_LAUNCH(2, 2);
#undef W_LAUNCH
  if (rc) return rc;
  return svlm_gemm_reduce_launch(partial, p.splits, bias, residual, ldr, C, ldc, M, N, act, norm_w, norm_b, eps, XN, ldxn, stream);
}

extern "C" int svlm_gemm_wfp8(const void* A, int lda, const void* W8, int ldw, const float* w_scale, const void* bias, const void* residual,
                              int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes, void* stream) {
  return gemm_wfp8_impl(A, lda, W8, ldw, w_scale, bias, residual, ldr, C, ldc, M, N, K, act, ws, ws_bytes, stream, nullptr, nullptr, 0.f, nullptr, 0);
}

extern "C" int svlm_gemm_wfp8_norm(const void* A, int lda, const void* W8, int ldw, const float* w_scale, const void* bias, const void* residual,
                                   int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes,
                                   const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn, void* stream) {
  SVLM_CHECK_ARG(norm_w != nullptr && XN != nullptr && N % 8 == 0 && ldc % 8 == 0 && ldxn % 8 == 0 && ldxn >= N && eps > 0.f,
                 "svlm_gemm_wfp8_norm: needs a norm weight, an output with 16-B aligned rows and N %% 8 == 0 (N=%d ldc=%d ldxn=%d)", N, ldc, ldxn);
  return gemm_wfp8_impl(A, lda, W8, ldw, w_scale, bias, residual, ldr, C, ldc, M, N, K, act, ws, ws_bytes, stream, norm_w, norm_b, eps, XN, ldxn);
}
