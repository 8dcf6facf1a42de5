// Weight-MXFP4, activation-bf16 MFMA GEMM:  C[M,N] = epi(A[M,K] . W'[N,K]^T),  W'[n,k] = e2m1(code[n,k]) * 2^(scale[n,k/32] - 127)
//   epi: the tile epilogues of gemm_tile.h (bias, activations 0..3, residual incl. in place, SVLM_ACT_SWIGLU on [gate rows; up rows],
//   split-K through the caller's workspace, the norm of the output row inside the split-K reduce); plan and launch: gemm_plan.h.
// The prefill of an `llm_fp4` engine reads the MXFP4 language-model weights with it instead of rebuilding every layer in bf16
// (svlm_dequant_fp4_bf16 + svlm_gemm_bf16).  The structure is gemm_wfp8_kernel's (gemm_wfp8.hip): the weight tile is staged as CODES,
// a quarter of the bytes of the bf16 image, and turned into bf16 when a wave reads its MFMA fragment -- once per W fragment, reused
// by all TM A fragments.  The block scale is a power of two and is applied inside the conversion (v_cvt_scalef32_pk_bf16_fp4), so
// code * scale is exact in bf16 and the MFMA sees bit for bit the operands the scratch path feeds it: with the same K per split the
// result EQUALS svlm_gemm_bf16 on the dequantised matrix (v_mfma_f32_16x16x32_bf16, same k -> lane mapping, same K order, same
// epilogue).  Layout of W4 and the scales: include/svlm.h above svlm_dec_qkv_fp4 (weights.py:quantize_blocks_mxfp4).
//
// Replaces (prefill rows of an fp4 language model): qwen2/language_forward.py:80-82,161 and Qwen2MLP (:201).
//
// Tile (16 TM WM) x 128 x 64, 2 WM waves as WM (m) x 2 (n).  LDS stage = A tile (BM rows x 128 B, the image of gemm_glds_kernel) +
// W tile (128 rows x 32 B of codes = 4 KiB, four 1-KiB DMA pieces: waves 0..3 issue one each, the 8-wave tile's waves 4..7 none).
//
// W tile layout and its conflict count.  A W row holds two 16-B chunks; chunk c of row r lives at position c ^ ((r >> 3) & 1).  A
// lane's fragment for K-step ks is 8 codes = 4 B at chunk ks, byte (fq * 4).  Read as ds_read_b32 (32 banks of 4 B, lane groups
// {0-31} = fq 0,1 and {32-63} = fq 2,3) a group covers 16 rows x 8 B on a 32-B row pitch: rows r, r+4, r+8, r+12 share their banks,
// and because the DMA places whole 16-B chunks the 16 rows of a group have only 8 distinct chunk positions modulo the 128 B of the
// banks: no chunk permutation gets below a 2-way conflict (4 LDS cycles per read instead of 2).  So the read is a ds_read_b64 of the
// 8-B half-chunk (fq / 2) that both lanes of a pair fq = 2p, 2p + 1 address (identical addresses broadcast): 64 banks of 4 B, a
// group covers 16 rows x 8 B = 32 banks, rows r and r + 8 are 256 B apart and the swizzle moves r + 8 to the other chunk ->
// conflict-free, 2 LDS cycles per read, and the lane keeps dword (fq & 1) with one v_cndmask.  The DMA image is lane-linear (1 KiB
// piece = 32 rows x 32 B, lane i -> row i / 2, position i % 2), so the swizzle sits on the per-lane SOURCE address and again on the
// fragment read.
//
// Block scales.  One e8m0 byte per (W row, K-step of 32): two bytes per fragment row per K-tile.  issue(kt) loads them with one 2-B
// global load per fragment row (4 per lane; 2-B aligned since K % 64 == 0 and the K per split is a multiple of 64) into one of three
// register sets that rotate with the ring (the K loop is unrolled by three so that the set index is static).  ONE TILE IN FLIGHT is
// therefore A_INST + (1 if the wave issues a W piece) DMA instructions + 4 scale loads, all vm operations that return in order; the
// hand-counted waits below count exactly that.
#include "common.h"
#include "gemm_plan.h"
#include "gemm_tile.h"
#include <stdlib.h>
#include <type_traits>

#define W4_BN 128
#define W4_BK 64

extern __shared__ __attribute__((aligned(16))) unsigned char wfp4_dyn_smem[];

#define W4_GLDS(gp, lp) \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp), (__attribute__((address_space(3))) void*)(lp), 16, 0, 0)

// 8 e2m1 codes (k ascending: byte 0 low nibble, byte 0 high nibble, byte 1 low nibble, ...) times 2^e -> 8 bf16, the MFMA fragment.
// v_cvt_scalef32_pk_bf16_fp4 converts the two codes of byte `byte_sel` and multiplies by the scale; a code has two significant bits
// and the scale is a power of two far inside the bf16 exponent range, so the rounding to bf16 never acts
// (tests/test_gemm_wfp4_gpu.py: all 16 codes at every position under five scale patterns).
__device__ __forceinline__ bf16x8_t wfp4_fragment(const unsigned c, const float scale) {
  u32x4_t o;
  o[0] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 0));
  o[1] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 1));
  o[2] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 2));
  o[3] = __builtin_bit_cast(unsigned, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(c, scale, 3));
  return __builtin_bit_cast(bf16x8_t, o);
}

template <int TM, int WM = 2>
__global__ __launch_bounds__(128 * WM) void gemm_wfp4_kernel(const bf16_t* __restrict__ A, int lda,
                                                             const unsigned char* __restrict__ W4, int ldw,
                                                             const unsigned char* __restrict__ w_scale,
                                                             const bf16_t* __restrict__ bias,
                                                             const bf16_t* residual, int ldr,
                                                             bf16_t* C, int ldc, float* __restrict__ partial,
                                                             int M, int N, int K, int k_per_split, int act, int gm, int gn, int splits) {
  constexpr int BM = 16 * TM * WM;
  constexpr int A_INST = TM;                    // 1-KiB DMA pieces per wave per tile: A (8 rows x 128 B each, BM / 8 pieces over 2 WM waves)
  constexpr int S_INST = 4;                     // 2-B scale loads per lane per tile (one per W fragment row)
  constexpr int STAGE_B = BM * 128 + W4_BN * 32;
  unsigned char* smem = wfp4_dyn_smem;

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // W: four pieces (32 rows x 32 B of codes each), one per wave 0..3.  Uniform (an SGPR), so that the waits below branch on the scalar unit
  const bool has_w = WM == 2 || __builtin_amdgcn_readfirstlane(wave) < 4;
  int tm, tn, split;
  if (!gemm_tile_of(blockIdx.x, gm, gn, splits, tm, tn, split)) return;
  const bool swiglu = act == SVLM_ACT_SWIGLU;     // 64 output columns per tile: gate | up halves of the 128 tile rows of W
  const int m0 = tm * BM, n0 = tn * (swiglu ? W4_BN / 2 : W4_BN);
  const int k_begin = split * k_per_split;
  const int k_end = min(K, k_begin + k_per_split);
  const int nk = (k_end - k_begin) / W4_BK;      // K % 64 == 0 and k_per_split % 64 == 0


  const bf16_t* a_src[A_INST];
#pragma unroll
  for (int i = 0; i < A_INST; ++i) {             // A piece: row = piece * 8 + lane / 8, position lane % 8 holds chunk p ^ (row & 7)
    const int row = (wave * A_INST + i) * 8 + (lane >> 3);
    a_src[i] = A + (size_t)min(m0 + row, M - 1) * lda + k_begin + (((lane & 7) ^ (row & 7)) * 8);
  }
  // W piece `wave` (waves 0..3): row = piece * 32 + lane / 2, position lane % 2 holds chunk p ^ ((row >> 3) & 1); 32 B of codes per K-tile
  const int wrow = (wave & 3) * 32 + (lane >> 1);
  const unsigned char* w_src = W4 + (size_t)w_row(wrow, n0, N, swiglu) * ldw + (k_begin >> 1) + (((lane & 1) ^ ((wrow >> 3) & 1)) * 16);
  const int fr = lane & 15, fq = lane >> 4;
  // the scale bytes of this lane's four W fragment rows: blocks (k_begin + 64 kt) / 32 and + 1 of a row are element kt of s_src[j]
  const unsigned short* s_src[S_INST];
#pragma unroll
  for (int j = 0; j < S_INST; ++j)
    s_src[j] = reinterpret_cast<const unsigned short*>(w_scale + (size_t)w_row(wn * 64 + j * 16 + fr, n0, N, swiglu) * (K >> 5) + (k_begin >> 5));
  unsigned sc[3][S_INST] = {};                   // one set per ring stage: low byte = K-step 0, high byte = K-step 1

  // one tile: A_INST (+ 1) DMA pieces and S_INST scale loads
  auto issue = [&](int kt, auto stage_c) {
    constexpr int stage = decltype(stage_c)::value;
    unsigned char* sa = smem + stage * STAGE_B;
    unsigned char* sw = sa + BM * 128;
#pragma unroll
    for (int i = 0; i < A_INST; ++i) W4_GLDS(a_src[i] + kt * W4_BK, sa + (wave * A_INST + i) * 1024);
    if (has_w) W4_GLDS(w_src + kt * (W4_BK / 2), sw + (wave & 3) * 1024);
    // The scale loads are written out: hipcc does not see the hand-counted waits, so for a load of its own it assumes every earlier
    // tile still in flight and, on the paths that issue no further tile, puts s_waitcnt vmcnt(0) in front of compute() -- right
    // behind the issue of the newest tile, which ends the ring.  What keeps this sound: a set's registers are written by these loads
    // only and first read in compute() of their own stage, behind the counted wait that covers them (the empty volatile asm there pins
    // that first read; volatile asm statements keep their order).  (global_load_ushort zero-extends into the 32-bit register.)
#pragma unroll
    for (int j = 0; j < S_INST; ++j) {
      const unsigned short* p = s_src[j] + kt;
      unsigned v;
      asm volatile("global_load_ushort %0, %1, off" : "=v"(v) : "v"(p) : "memory");
      sc[stage][j] = v;
    }
  };

  f32x4_t acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // byte offsets of this lane's W fragments inside a stage's W tile: codes k = ks * 32 + fq * 8 .. + 7 are dword fq of chunk ks; the read
  // takes the 8-B half (fq / 2) of that chunk.  Each offset is made opaque so that the reads stay eight ds_read_b64: with a common base
  // hipcc pairs them into ds_read2st64_b64, which moves a quarter of the bytes per LDS cycle (32-bank mode).
  unsigned woff[2][4];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      woff[ks][j] = (wn * 64 + j * 16 + fr) * 32 + ((ks ^ ((fr >> 3) & 1)) * 16) + (fq >> 1) * 8;
      asm volatile("" : "+v"(woff[ks][j]));
    }
  const bool odd = fq & 1;
  auto compute = [&](auto stage_c) {
    constexpr int stage = decltype(stage_c)::value;
    const unsigned char* sa = smem + stage * STAGE_B;
    const unsigned char* sw = sa + BM * 128;
    // the scale registers are first touched here, behind the hand-counted wait that covered their loads (volatile asm keeps its order)
#pragma unroll
    for (int j = 0; j < S_INST; ++j) {
      unsigned v = sc[stage][j];
      asm volatile("" : "+v"(v));
      sc[stage][j] = v;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8_t af[TM], wf[4];
      const int pos = ((ks * 4 + fq) ^ (fr & 7)) * 16;      // rows of a fragment differ by multiples of 16 -> row & 7 == fr & 7
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const bf16x8_t*>(sa + (wm * 16 * TM + i * 16 + fr) * 128 + pos);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x2_t pr = *reinterpret_cast<const u32x2_t*>(sw + woff[ks][j]);
        // the scale as the float the conversion multiplies with: byte << 23 (dec_fp4.h:e8m0_f32)
        const float s = __uint_as_float(ks ? (sc[stage][j] >> 8) << 23 : (sc[stage][j] & 0xFFu) << 23);
        wf[j] = wfp4_fragment(odd ? pr[1] : pr[0], s);
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], af[i], acc[i][j], 0, 0, 0);
    }
  };

  // 3-stage ring, 2 tiles in flight; waits counted by hand, raw barrier.  Leaving the newer tile in flight means leaving its
  // A_INST + 1 + S_INST vm operations (A_INST + S_INST in a wave that issues no W piece) outstanding.
  auto step = [&](int kt, auto stage_c) {
    constexpr int stage = decltype(stage_c)::value;
    if (kt + 1 < nk) {
      if (has_w) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_INST + 1 + S_INST) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(A_INST + S_INST) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    asm volatile("s_barrier" ::: "memory");
    if (kt + 2 < nk) issue(kt + 2, std::integral_constant<int, (stage + 2) % 3>{});
    compute(stage_c);
  };
  issue(0, std::integral_constant<int, 0>{});          // nk >= 1
  if (1 < nk) issue(1, std::integral_constant<int, 1>{});
  for (int kt = 0; kt < nk; kt += 3) {
    step(kt, std::integral_constant<int, 0>{});          // (one exit: with a break between the steps the accumulators get copies per exit)
    if (kt + 1 < nk) step(kt + 1, std::integral_constant<int, 1>{});
    if (kt + 2 < nk) step(kt + 2, std::integral_constant<int, 2>{});
  }

  if (swiglu) {
    gemm_tile_epilogue_swiglu<TM>(acc, smem, m0, n0, wm, wn, fr, fq, M, N, bias, C, ldc);
    return;
  }
  gemm_tile_epilogue<TM>(acc, m0, n0, wm, wn, fr, fq, split, M, N, bias, residual, ldr, C, ldc, partial, act);
}

static int gemm_wfp4_impl(const void* A, int lda, const void* W4, int ldw, const void* w_scale, const void* bias, const void* residual, int ldr,
                          void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes, void* stream,
                          const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn) {
  SVLM_CHECK_ARG(M >= 0 && N > 0 && K > 0, "svlm_gemm_wfp4: bad shape M=%d N=%d K=%d", M, N, K);
  SVLM_CHECK_ARG(K % W4_BK == 0 && N % 4 == 0, "svlm_gemm_wfp4: K=%d must be a multiple of 64 and N=%d of 4", K, N);
  SVLM_CHECK_ARG(W4 != nullptr && ((uintptr_t)W4 & 15) == 0, "svlm_gemm_wfp4: needs 16-B aligned codes");
  SVLM_CHECK_ARG(w_scale != nullptr && ((uintptr_t)w_scale & 1) == 0,
                 "svlm_gemm_wfp4: needs 2-B aligned e8m0 scales, one byte per block of 32 ([rows of W4, K / 32], contiguous)");
  SVLM_CHECK_ARG(lda % 8 == 0 && ldw % 16 == 0 && ldc % 4 == 0 && (!residual || ldr % 4 == 0),
                 "svlm_gemm_wfp4: leading dims must keep 16-B row alignment (lda=%d ldw=%d bytes ldc=%d ldr=%d)", lda, ldw, ldc, ldr);
  SVLM_CHECK_ARG(lda >= K && ldw >= K / 2 && ldc >= N, "svlm_gemm_wfp4: leading dim smaller than row length (ldw is in bytes, K / 2 per row)");
  SVLM_CHECK_ARG(act >= 0 && act <= 4, "svlm_gemm_wfp4: unknown activation %d", act);
  const bool swiglu = act == SVLM_ACT_SWIGLU;
  SVLM_CHECK_ARG(!swiglu || (residual == nullptr && norm_w == nullptr && N % 8 == 0),
                 "svlm_gemm_wfp4: SVLM_ACT_SWIGLU takes W4 = [gate; up] (scales and bias = [gate; up] too) without residual or norm, N %% 8 == 0 (N=%d)", N);
  if (M == 0) return SVLM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int gn = swiglu ? (N + W4_BN / 2 - 1) / (W4_BN / 2) : (N + W4_BN - 1) / W4_BN;
  // ---- tile height and K-split: the plan of svlm_gemm_bf16 on this kernel's tiles (gemm_plan.h:gemm_wcode_plan; a shape gets the K
  // per split its bf16 twin gets and reproduces it bit for bit), which also writes the plan note
  const GemmWPlan p = gemm_wcode_plan("SVLM_GEMM_WFP4", 3, M, N, K, gn, swiglu, ws, ws_bytes);
  float* partial = p.splits > 1 ? (float*)ws : nullptr;
  // LDS: three stages of A tile (BM rows x 128 B) + W tile of codes
#define W_LAUNCH(TM, WM)                                                                                                                   \
  gemm_launch<&gemm_wfp4_kernel<TM, WM>, 128 * WM, 3 * (16 * TM * WM * 128 + W4_BN * 32)>("svlm_gemm_wfp4", p.nblocks, st, A, lda, W4, ldw, w_scale, bias, residual, \
                                                                                  ldr, C, ldc, partial, M, N, K, p.kps, act, p.gm, gn, p.splits)
  const int rc = p.bm == 256 ? W_LAUNCH(4, 4) : p.bm == 128 ? W_LAUNCH(4, 2) : W_LAUNCH(2, 2);
#undef W_LAUNCH
  if (rc) return rc;
  return svlm_gemm_reduce_launch(partial, p.splits, bias, residual, ldr, C, ldc, M, N, act, norm_w, norm_b, eps, XN, ldxn, stream);
}

extern "C" int svlm_gemm_wfp4(const void* A, int lda, const void* W4, int ldw, const void* w_scale, const void* bias, const void* residual,
                              int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes, void* stream) {
  return gemm_wfp4_impl(A, lda, W4, ldw, w_scale, bias, residual, ldr, C, ldc, M, N, K, act, ws, ws_bytes, stream, nullptr, nullptr, 0.f, nullptr, 0);
}

extern "C" int svlm_gemm_wfp4_norm(const void* A, int lda, const void* W4, int ldw, const void* w_scale, const void* bias, const void* residual,
                                   int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes,
                                   const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn, void* stream) {
  SVLM_CHECK_ARG(norm_w != nullptr && XN != nullptr && N % 8 == 0 && ldc % 8 == 0 && ldxn % 8 == 0 && ldxn >= N && eps > 0.f,
                 "svlm_gemm_wfp4_norm: needs a norm weight, an output with 16-B aligned rows and N %% 8 == 0 (N=%d ldc=%d ldxn=%d)", N, ldc, ldxn);
  return gemm_wfp4_impl(A, lda, W4, ldw, w_scale, bias, residual, ldr, C, ldc, M, N, K, act, ws, ws_bytes, stream, norm_w, norm_b, eps, XN, ldxn);
}
