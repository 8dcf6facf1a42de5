// MX prefill GEMM on the block-scaled MFMA:  C[M,N] = epi(A'[M,K] . W'[N,K]^T)
//   A'[m,k] = e4m3(A8[m,k]) * 2^(a_scale[m,k/32] - 127)      MXFP8 activations (svlm_quant_mxfp8 below; weights.py:quantize_blocks_mxfp8)
//   W'[n,k] = e2m1(W4[n,k]) * 2^(w_scale[n,k/32] - 127)      the MXFP4 language-model weights as EngineWeights holds them
//   epi: the tile epilogues of gemm_tile.h (bias, activations 0..3, residual incl. in place, SVLM_ACT_SWIGLU on [gate rows; up rows],
//   split-K through the caller's workspace, the norm of the output row inside the split-K reduce); plan and launch: gemm_plan.h.
// Both A' and W' are exactly representable in bf16 and every product is exact in fp32, so this is svlm_gemm_bf16 on (A', W') up to the
// fp32 summation order.  The reference has bf16 activations; the rounding of the activations to e4m3 per block of 32 is this mode's
// own numeric definition (opt-in: SvlmEngine(llm_fp4=True, prefill_mx=True)).
//
// Replaces (prefill rows of an fp4 language model): qwen2/language_forward.py:80-82,161 and Qwen2MLP (:201).
//
// Structure: gemm_fp8_kernel's (gemm_fp8.hip) -- (32 TM) x 128 tile, K-step 128, 3-stage global_load_lds ring, counted vmcnt + raw
// barrier, 4 waves as 2 (m) x 2 (n) -- with ONE v_mfma_scale_f32_16x16x128_f8f6f4 per fragment pair and K-step, the fp4 format on the
// weight operand (first operand, cbsz 4: 4 VGPRs of codes) and e4m3 on the activation operand (8 VGPRs).
//
// Operand layout of the scaled MFMA (16x16x128) with an fp4 and an e4m3 operand, as established on the hardware (a one-wave probe
// with one-hot operands and one scale value per lane group; tests/test_gemm_mx_gpu.py pins it): lane (fr = lane % 16, fq = lane / 16)
// holds row fr of its operand.  The K-step's 128 k are four blocks of 32 consecutive k, and for BOTH operands the scale of block j of
// row fr is byte `op_sel` of the scale register of lane (fr, fq = j).  The DATA of a block sits elsewhere per format:
//   e2m1: lane fq holds k = 32 fq .. 32 fq + 31 in its 4 VGPRs, ascending from byte 0, the even k in the LOW nibble -- block fq, the
//         block its own scale register describes;
//   e4m3: lane fq holds k = 16 fq .. 16 fq + 15 in VGPRs 0-3 and k = 64 + 16 fq .. 64 + 16 fq + 15 in VGPRs 4-7, ascending bytes (the
//         two passes of 64 k the instruction makes over an 8-bit operand): the 16-B chunks fq and 4 + fq of the row, which is what
//         gemm_fp8_kernel reads too.  Block j is spread over the lanes 2 (j % 2) and 2 (j % 2) + 1; its scale still comes from lane j.
// So a lane's e4m3 values are NOT the block its scale byte describes, and a lane that fetched "its" 32 consecutive k (chunks 2 fq and
// 2 fq + 1) would be multiplied with the wrong weights.  op_sel is an immediate, so every lane puts the scale byte of (its row, block
// fq) into byte 0 of its register.
//
// LDS stage = A tile (BM rows x 128 B) + W tile (128 rows x 64 B of codes) + scales (BM + 128 rows x 4 B, one byte per block of the
// K-step).  A row: eight 16-B chunks, chunk c at position c ^ (row & 7); a lane reads chunks fq and 4 + fq.  W row: four 16-B
// chunks, chunk c at position c ^ ((row >> 2) & 3); a lane reads chunk fq: the 16 lanes of a ds_read_b128 pass (16 rows on a 64-B
// pitch) cover four distinct 64-B windows (row & 3) x four distinct positions: all 64 banks once.  The scale bytes of a K-step are 4
// contiguous bytes per row in global memory (K % 128 == 0): one 4-B global_load_lds per row; a lane reads its byte with ds_read_u8.
// One tile in flight = TM (A) + 2 (W) + 1 (scales) DMA instructions per wave, which is what the waits count.
#include "common.h"
#include "gemm_plan.h"
#include "gemm_tile.h"
#include <stdlib.h>

#define MX_BN 128
#define MX_BK 128           // elements per K-step: 128 B of e4m3 per A row, 64 B of e2m1 codes per W row, 4 scale bytes per row

extern __shared__ __attribute__((aligned(16))) unsigned char gemm_mx_dyn_smem[];

#define MX_GLDS(gp, lp, nbytes) \
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(gp), (__attribute__((address_space(3))) void*)(lp), nbytes, 0, 0)

typedef int mx_i8x_t __attribute__((ext_vector_type(8)));
typedef int mx_i4x_t __attribute__((ext_vector_type(4)));

template <int TM>
__global__ __launch_bounds__(256) void gemm_mx_kernel(const unsigned char* __restrict__ A, int lda, const unsigned char* __restrict__ a_scale,
                                                      const unsigned char* __restrict__ W4, int ldw, const unsigned char* __restrict__ w_scale,
                                                      const bf16_t* __restrict__ bias, const bf16_t* residual, int ldr,
                                                      bf16_t* C, int ldc, float* __restrict__ partial,
                                                      int M, int N, int K, int k_per_split, int act, int gm, int gn, int splits) {
  constexpr int BM = 32 * TM;
  constexpr int A_INST = TM;                     // 1-KiB A pieces per wave per tile (8 rows x 128 B each)
  constexpr int W_INST = 2;                      // 1-KiB W pieces per wave per tile (16 rows x 64 B each)
  constexpr int NPT = A_INST + W_INST + 1;       // + one 256-B piece of scales
  constexpr int A_B = BM * 128, W_B = MX_BN * 64;
  constexpr int STAGE_B = A_B + W_B + 1024;      // scales: [A rows 0..127 x 4 B][W rows 0..127 x 4 B]
  constexpr int NS = 3;
  unsigned char* smem = gemm_mx_dyn_smem;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  int tm, tn, split;
  if (!gemm_tile_of(blockIdx.x, gm, gn, splits, tm, tn, split)) return;
  const bool swiglu = act == SVLM_ACT_SWIGLU;     // 64 output columns per tile: gate | up halves of the 128 tile rows of W
  const int m0 = tm * BM, n0 = tn * (swiglu ? MX_BN / 2 : MX_BN);
  const int k_begin = split * k_per_split;
  const int k_end = min(K, k_begin + k_per_split);
  const int nk = (k_end - k_begin) / MX_BK;       // K % 128 == 0 and k_per_split % 128 == 0
  const int nb = K >> 5;                          // scale bytes per row


  const unsigned char* a_src[A_INST];
  const unsigned char* w_src[W_INST];
#pragma unroll
  for (int i = 0; i < A_INST; ++i) {              // A piece: row = piece * 8 + lane / 8, position lane % 8 holds chunk p ^ (row & 7)
    const int row = (wave * A_INST + i) * 8 + (lane >> 3);
    a_src[i] = A + (size_t)min(m0 + row, M - 1) * lda + k_begin + (((lane & 7) ^ (row & 7)) * 16);
  }
#pragma unroll
  for (int i = 0; i < W_INST; ++i) {              // W piece: row = piece * 16 + lane / 4, position lane % 4 holds chunk p ^ ((row >> 2) & 3)
    const int row = (wave * W_INST + i) * 16 + (lane >> 2);
    w_src[i] = W4 + (size_t)w_row(row, n0, N, swiglu) * ldw + (k_begin >> 1) + (((lane & 3) ^ ((row >> 2) & 3)) * 16);
  }
  // scales: waves 0, 1 bring the A rows 64 wave + lane (the second piece of a 64-row tile lands unused), waves 2, 3 the W rows
  const unsigned char* s_src = wave < 2 ? a_scale + (size_t)min(m0 + wave * 64 + lane, M - 1) * nb + (k_begin >> 5)
                                        : w_scale + (size_t)w_row((wave - 2) * 64 + lane, n0, N, swiglu) * nb + (k_begin >> 5);
  auto issue = [&](int kt, int stage) {
    unsigned char* sa = smem + stage * STAGE_B;
    unsigned char* sw = sa + A_B;
    unsigned char* ss = sw + W_B;
#pragma unroll
    for (int i = 0; i < A_INST; ++i) MX_GLDS(a_src[i] + kt * MX_BK, sa + (wave * A_INST + i) * 1024, 16);
#pragma unroll
    for (int i = 0; i < W_INST; ++i) MX_GLDS(w_src[i] + kt * (MX_BK / 2), sw + (wave * W_INST + i) * 1024, 16);
    MX_GLDS(s_src + kt * 4, ss + wave * 256, 4);
  };
  f32x4_t acc[TM][4];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  const int fr = lane & 15, fq = lane >> 4;
  // rows of a fragment differ by multiples of 16 -> row & 7 == fr & 7 and (row >> 2) & 3 == (fr >> 2) & 3
  const int ap0 = (fq ^ (fr & 7)) * 16, ap1 = ((4 + fq) ^ (fr & 7)) * 16;      // e4m3: k = 16 fq .. and 64 + 16 fq .. (see above)
  const int wp = (fq ^ ((fr >> 2) & 3)) * 16;
  auto compute = [&](int stage) {
    const unsigned char* sa = smem + stage * STAGE_B;
    const unsigned char* sw = sa + A_B;
    const unsigned char* ss = sw + W_B;
    mx_i8x_t af[TM], wf[4];
    int as[TM], wsc[4];
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      const int row = wm * 16 * TM + i * 16 + fr;
      const unsigned char* r = sa + row * 128;
      const mx_i4x_t lo = *reinterpret_cast<const mx_i4x_t*>(r + ap0), hi = *reinterpret_cast<const mx_i4x_t*>(r + ap1);
      af[i] = mx_i8x_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
      as[i] = ss[row * 4 + fq];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = wn * 64 + j * 16 + fr;
      const mx_i4x_t c = *reinterpret_cast<const mx_i4x_t*>(sw + row * 64 + wp);
      wf[j] = mx_i8x_t{c[0], c[1], c[2], c[3], 0, 0, 0, 0};
      wsc[j] = ss[512 + row * 4 + fq];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(wf[j], af[i], acc[i][j], 4, 0, 0, wsc[j], 0, as[i]);
  };
  constexpr int AHEAD = NS - 1;
#pragma unroll
  for (int t = 0; t < AHEAD; ++t)
    if (t < nk) issue(t, t);
  for (int kt = 0; kt < nk; ++kt) {
    const int newer = min(AHEAD - 1, nk - 1 - kt);
    if (newer >= 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(NPT) : "memory");
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

// ---------------------------------------------------------------- row quantiser: bf16 (rows, cols) -> MXFP8 (e4m3 codes + e8m0 per 32)
// weights.py:quantize_blocks_mxfp8, bit for bit.  Two lanes per block, 16 elements each (two 16-B loads, one 16-B store); the amax is
// taken on the bf16 magnitudes as integers (monotonic, and an inf / NaN is >= 0x7F80) with one DPP step between the two lanes.  With
// amax = 1.f * 2^E: e = E - 8 if the 7 mantissa bits are <= 0x60 (m = 1.f / 2 <= 0.875) else E - 7, clamped below at -117 (a
// subnormal amax lands there whatever its bits say), 0 for an all-zero block.  x * 2^-e is exact in fp32 (-e in [-120, 117]).
__global__ __launch_bounds__(256) void quant_mxfp8_kernel(const bf16_t* __restrict__ x, int ldx, unsigned char* __restrict__ q, int ldq,
                                                          unsigned char* __restrict__ scale, int rows, int cols) {
  const int hpr = cols >> 4;                                           // half blocks per row (even)
  const size_t h = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (h >= (size_t)rows * hpr) return;                                 // (the two lanes of a block leave together)
  const int row = (int)(h / hpr), c = (int)(h % hpr) * 16;
  const u32x4_t* src = reinterpret_cast<const u32x4_t*>(x + (size_t)row * ldx + c);
  const u32x4_t v0 = src[0], v1 = src[1];
  unsigned mx = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    mx = max(mx, max(v0[i] & 0x7FFFu, (v0[i] >> 16) & 0x7FFFu));
    mx = max(mx, max(v1[i] & 0x7FFFu, (v1[i] >> 16) & 0x7FFFu));
  }
  mx = max(mx, (unsigned)__builtin_amdgcn_update_dpp(0u, mx, 0xB1, 0xF, 0xF, true));      // quad_perm [1,0,3,2]: the block's other half
  u32x4_t o;
  int sbyte;
  if (mx >= 0x7F80u) {                                                 // an inf or a NaN in the block: all NaN codes, scale 2^0
    o = u32x4_t{0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu, 0x7F7F7F7Fu};
    sbyte = 127;
  } else {
    int e = (int)(mx >> 7) - 127 - ((mx & 0x7Fu) <= 0x60u ? 8 : 7);
    e = mx == 0 ? 0 : max(e, -117);
    sbyte = e + 127;
    const float inv = __uint_as_float((unsigned)(127 - e) << 23);      // 2^-e, a normal fp32
    float f[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[2 * i] = lo_bf(v0[i]) * inv; f[2 * i + 1] = hi_bf(v0[i]) * inv;
      f[8 + 2 * i] = lo_bf(v1[i]) * inv; f[8 + 2 * i + 1] = hi_bf(v1[i]) * inv;
    }
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      int p = 0;
      p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w], f[4 * w + 1], p, false);
      p = __builtin_amdgcn_cvt_pk_fp8_f32(f[4 * w + 2], f[4 * w + 3], p, true);
      o[w] = (unsigned)p;
    }
  }
  *reinterpret_cast<u32x4_t*>(q + (size_t)row * ldq + c) = o;
  if ((c & 16) == 0) scale[(size_t)row * (cols >> 5) + (c >> 5)] = (unsigned char)sbyte;
}

extern "C" int svlm_quant_mxfp8(const void* x, int ldx, void* q, int ldq, void* scale, int rows, int cols, void* stream) {
  SVLM_CHECK_ARG(rows >= 0 && cols > 0 && cols % 32 == 0 && ldx % 8 == 0 && ldq % 16 == 0 && ldx >= cols && ldq >= cols,
                 "svlm_quant_mxfp8: bad shape rows=%d cols=%d ldx=%d ldq=%d (cols a multiple of 32, rows 16-B aligned)", rows, cols, ldx, ldq);
  SVLM_CHECK_ARG(rows == 0 || (x != nullptr && q != nullptr && scale != nullptr && ((uintptr_t)x & 15) == 0 && ((uintptr_t)q & 15) == 0),
                 "svlm_quant_mxfp8: needs 16-B aligned rows, codes and a scale array ([rows, cols / 32] bytes, contiguous)");
  if (rows == 0) return SVLM_OK;
  const size_t total = (size_t)rows * (cols >> 4);
  quant_mxfp8_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>((const bf16_t*)x, ldx, (unsigned char*)q, ldq,
                                                                                       (unsigned char*)scale, rows, cols);
  return svlm_check_launch("svlm_quant_mxfp8");
}

static int gemm_mx_impl(const void* A8, int lda, const void* a_scale, const void* W4, int ldw, const void* w_scale, const void* bias,
                        const void* residual, int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes,
                        void* stream, const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn) {
  SVLM_CHECK_ARG(M >= 0 && N > 0 && K > 0, "svlm_gemm_mx_a8w4: bad shape M=%d N=%d K=%d", M, N, K);
  SVLM_CHECK_ARG(K % MX_BK == 0 && N % 4 == 0, "svlm_gemm_mx_a8w4: K=%d must be a multiple of 128 and N=%d of 4", K, N);
  SVLM_CHECK_ARG(A8 != nullptr && ((uintptr_t)A8 & 15) == 0 && W4 != nullptr && ((uintptr_t)W4 & 15) == 0,
                 "svlm_gemm_mx_a8w4: needs 16-B aligned e4m3 and e2m1 codes");
  SVLM_CHECK_ARG(a_scale != nullptr && ((uintptr_t)a_scale & 3) == 0 && w_scale != nullptr && ((uintptr_t)w_scale & 3) == 0,
                 "svlm_gemm_mx_a8w4: needs 4-B aligned e8m0 scales, one byte per block of 32 ([M, K / 32] and [rows of W4, K / 32], contiguous)");
  SVLM_CHECK_ARG(lda % 16 == 0 && ldw % 16 == 0 && ldc % 4 == 0 && (!residual || ldr % 4 == 0),
                 "svlm_gemm_mx_a8w4: leading dims must keep 16-B row alignment (lda=%d ldw=%d bytes ldc=%d ldr=%d)", lda, ldw, ldc, ldr);
  SVLM_CHECK_ARG(lda >= K && ldw >= K / 2 && ldc >= N, "svlm_gemm_mx_a8w4: leading dim smaller than row length (lda and ldw are in bytes, K and K / 2 per row)");
  SVLM_CHECK_ARG(act >= 0 && act <= 4, "svlm_gemm_mx_a8w4: unknown activation %d", act);
  SVLM_CHECK_ARG(C != nullptr && (bias == nullptr || ((uintptr_t)bias & 7) == 0) && ((uintptr_t)C & 7) == 0 && (!residual || ((uintptr_t)residual & 7) == 0),
                 "svlm_gemm_mx_a8w4: needs an output, and 8-B aligned output, bias and residual");
  const bool swiglu = act == SVLM_ACT_SWIGLU;
  SVLM_CHECK_ARG(!swiglu || (residual == nullptr && norm_w == nullptr && N % 8 == 0),
                 "svlm_gemm_mx_a8w4: SVLM_ACT_SWIGLU takes W4 = [gate; up] (scales and bias = [gate; up] too) without residual or norm, N %% 8 == 0 (N=%d)", N);
  if (M == 0) return SVLM_OK;
  hipStream_t st = (hipStream_t)stream;
  const int gn = swiglu ? (N + MX_BN / 2 - 1) / (MX_BN / 2) : (N + MX_BN - 1) / MX_BN;
  // ---- plan (tests/gemm_mx_paths.py:plan_mx is its mirror).  Tile rows: 128 from 1024 rows on (a 4096-row pass of a dense prefill
  // reads each W tile half as often), 64 below (chunk prefills of 290..590 rows: more workgroups).  K-split, 64-row tiles only: while
  // the tile grid is below two workgroups per CU (512), up to that many, at least 512 of K per split, at most 8 slabs; the 4096-row
  // passes fill the CUs un-split.  A fused norm rides in the split-K reduce, so a GEMM with a norm takes two splits where it would take one.
  int bm = M >= 1024 ? 128 : 64;
  int splits = 1;
  const bool can_split = ws != nullptr && !swiglu;
  const long long tiles = (long long)((M + bm - 1) / bm) * gn;
  if (can_split && bm == 64 && tiles < 512 && K >= 1024) {
    splits = (int)((512 + tiles - 1) / tiles);
    if (splits > K / 512) splits = K / 512;
    if (splits > 8) splits = 8;
    while (splits > 1 && (long long)splits * M * N * 4 > ws_bytes) --splits;
  }
  if (const char* fb = svlm_env("SVLM_GEMM_MX_BM")) { const int v = atoi(fb); if (v == 64 || v == 128) bm = v; }
  if (const char* fs = svlm_env("SVLM_GEMM_MX_SPLITS")) {
    const int v = atoi(fs);
    if (v == 1 || (v > 1 && v <= K / MX_BK && can_split && (long long)v * M * N * 4 <= ws_bytes)) splits = v;
  }
  if (norm_w != nullptr && splits == 1 && can_split && K >= 2 * MX_BK && (long long)2 * M * N * 4 <= ws_bytes && N <= 4096) splits = 2;
  int kps;
  gemm_finish_split(K, MX_BK, &splits, &kps);
  const int gm = (M + bm - 1) / bm;
  float* partial = splits > 1 ? (float*)ws : nullptr;
  const int nblocks = gemm_grid_size(gm, gn, splits);
  SVLM_DIAG(g_svlm_gemm_plan_note = SvlmGemmPlanNote{g_svlm_gemm_plan_note.seq + 1, 4, bm, 4, 3, 1, splits, kps, 0, 0});
  // LDS: three stages of A tile + W tile of codes + 1 KiB of scales
#define MX_LAUNCH(TM)                                                                                                                        \
  gemm_launch<&gemm_mx_kernel<TM>, 256, 3 * (32 * TM * 128 + MX_BN * 64 + 1024)>("svlm_gemm_mx_a8w4", nblocks, st, A8, lda, a_scale, W4, ldw, w_scale, \
                                                                                 bias, residual, ldr, C, ldc, partial, M, N, K, kps, act, gm, gn, splits)
  const int rc = bm == 128 ? MX_LAUNCH(4) : MX_LAUNCH(2);
#undef MX_LAUNCH
  if (rc) return rc;
  return svlm_gemm_reduce_launch(partial, splits, bias, residual, ldr, C, ldc, M, N, act, norm_w, norm_b, eps, XN, ldxn, stream);
}

extern "C" int svlm_gemm_mx_a8w4(const void* A8, int lda, const void* a_scale, const void* W4, int ldw, const void* w_scale, const void* bias,
                                 const void* residual, int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes,
                                 void* stream) {
  return gemm_mx_impl(A8, lda, a_scale, W4, ldw, w_scale, bias, residual, ldr, C, ldc, M, N, K, act, ws, ws_bytes, stream, nullptr, nullptr, 0.f,
                      nullptr, 0);
}

extern "C" int svlm_gemm_mx_a8w4_norm(const void* A8, int lda, const void* a_scale, const void* W4, int ldw, const void* w_scale, const void* bias,
                                      const void* residual, int ldr, void* C, int ldc, int M, int N, int K, int act, void* ws, long long ws_bytes,
                                      const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn, void* stream) {
  SVLM_CHECK_ARG(norm_w != nullptr && XN != nullptr && N % 8 == 0 && ldc % 8 == 0 && ldxn % 8 == 0 && ldxn >= N && eps > 0.f,
                 "svlm_gemm_mx_a8w4_norm: needs a norm weight, an output with 16-B aligned rows and N %% 8 == 0 (N=%d ldc=%d ldxn=%d)", N, ldc, ldxn);
  return gemm_mx_impl(A8, lda, a_scale, W4, ldw, w_scale, bias, residual, ldr, C, ldc, M, N, K, act, ws, ws_bytes, stream, norm_w, norm_b, eps, XN, ldxn);
}
