// Decode-step (T = 1) weight-streaming GEMVs on OCP MXFP4 weights: e2m1 codes, two per byte, with one e8m0 power-of-two scale per
// block of 32 K elements (the opt-in `llm_fp4` engine, weights.py:quantize_blocks_mxfp4).  The fused kernels are the SHELLS of the
// fp8 / bf16 ones (dec_shell.h) over the policy WFp4 (dec_fp4.h) -- one prologue, one epilogue (dec_epi.h), the same rounding points --
// around this file's K loop (fma_batch4, wave_dots4); the plain GEMV and the dequantisation are this file's own.  Entry, counterparts:
//
//   svlm_dec_qkv_fp4        svlm_dec_qkv_fp8      / svlm_dec_qkv_lin   RMSNorm -> QKV + bias -> K/V append (+ linear planes)
//   svlm_dec_gate_up_fp4    svlm_dec_gate_up_fp8  / svlm_dec_gate_up   RMSNorm -> gate/up -> SwiGLU
//   svlm_gemv_fp4           svlm_gemv_fp8         / svlm_gemv_bf16     o_proj / down_proj + residual
//   svlm_dequant_fp4_bf16   svlm_dequant_fp8_bf16                      code * 2^e -> bf16, the prefill's scratch layer
//
// (The lm_head of an fp4 engine stays e4m3 and goes through the fp8 head kernels.)
//
// W' = code * 2^e is exact in bf16 and every product code * 2^e * x is exact in fp32 (2 significant bits times 8), so each kernel
// computes the bf16 kernel on W' up to the fp32 summation order.  The scale is applied inside the conversion
// (v_cvt_scalef32_pk_f32_fp4), where it costs nothing.
//
// Structure: the fp8 kernels' with the K-step doubled.  One 16-B load carries 32 codes = one MX block, so a lane fetches one scale
// byte per load (64 consecutive bytes per wave, row and K-step) and nothing is shared across lanes; every load of a batch, scale
// bytes included, is issued before the first FMA; the normalised activation row is staged in LDS behind LDS-only barriers.  A lane owns
// 32 consecutive K elements per K-step, a K-step is 2048 elements, so the rows of the 2B / 3B / 7B models (K = 1536 / 2048 / 3584) are
// one or two K-steps: PRE is 1 or 2 (the whole row in flight before the first FMA), and the rows per wave are the most that keep a
// SIMD at 6 - 8 waves (launchers below: the VGPR counts of each choice), which is what keeps >= 32 KiB of loads in flight per CU.  The
// 32 activations of a lane's K-step are converted 16 at a time, each half shared by the wave's rows.
#include "common.h"
#include "dec_xrow.h"
#include "dec_fp4.h"
#include "dec_launch.h"           // host side: lane-count switch, qkv argument checks
#include "dec_shell.h"            // the kernel shells over WFp4 (dec_fp4.h); epilogue pieces: dec_epi.h

// ---------------------------------------------------------------- fused decode kernels (x staged in LDS)
template <int NR, int PRE>
__device__ __forceinline__ void fma_batch4(const W4Pre<NR, PRE>& pre, const bf16_t* xs, int base, int K, float (&acc)[NR]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 2048 + lane * 32;
    float s[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) s[r] = e8m0_f32(pre.s[it][r]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      float xf[16];
      x16(xs, c + 16 * h, K, xf);                            // K % 32 == 0: both halves of a block are inside K or neither is
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[r] = dot16_fp4(pre.w[it][r][2 * h], pre.w[it][r][2 * h + 1], s[r], xf, acc[r]);
    }
  }
}

// acc[r] = sum_k W'[row r][k] * xs[k] for NR rows of one wave; `pre` holds K-steps [0, PRE) already in flight
template <int NR, int PRE>
__device__ __forceinline__ void wave_dots4(const fp4x2_t* const (&wr)[NR], const e8m0_t* const (&sr)[NR], const bf16_t* xs, int K,
                                           float (&acc)[NR], W4Pre<NR, PRE>& pre) {
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.f;
  fma_batch4<NR, PRE>(pre, xs, 0, K, acc);
  for (int base = PRE * 2048; base < K; base += PRE * 2048) {
    preload_w4<NR, PRE>(wr, sr, base, K, pre);
    __builtin_amdgcn_sched_barrier(0);                       // every load of the batch is issued before its first FMA
    fma_batch4<NR, PRE>(pre, xs, base, K, acc);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = wave_sum(acc[r]);
}

template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_qkv_fp4_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                          const fp4x2_t* __restrict__ W, int ldw, const e8m0_t* __restrict__ S,
                                                          const bf16_t* __restrict__ bias, bf16_t* __restrict__ q_out,
                                                          bf16_t* __restrict__ k_planes, bf16_t* __restrict__ v_planes,
                                                          const int* __restrict__ slot_of, const int* __restrict__ len_dev, int len_host,
                                                          int N, int K, int qd, int kd, int D, int n_slots, bf16_t* __restrict__ k_lin,
                                                          bf16_t* __restrict__ v_lin, int lin_rows) {
  dec_qkv_body<WFp4, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, S, bias, q_out, k_planes, v_planes, slot_of, len_dev, len_host, N, K, qd, kd, D, n_slots,
                                    k_lin, v_lin, lin_rows);
}

template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_gate_up_fp4_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                              const fp4x2_t* __restrict__ W, int ldw, const e8m0_t* __restrict__ S,
                                                              bf16_t* __restrict__ h, int I, int K) {
  dec_gate_up_body<WFp4, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, S, h, I, K);
}

// ---------------------------------------------------------------- plain GEMV (x from global), optional K split over the waves
// The 4 waves of a workgroup form 4 / KW groups of ROWS rows each; the KW waves of a group take one 1/KW share of K each, a whole
// number of blocks (KW = 4: the long-K form of svlm_gemv_fp8, for a skinny output with a long reduction).
template <int ROWS, int KW, int PRE>
__global__ __launch_bounds__(256) void gemv_fp4_kernel(const bf16_t* __restrict__ x, const fp4x2_t* __restrict__ W, int ldw,
                                                       const e8m0_t* __restrict__ S, const bf16_t* __restrict__ bias,
                                                       const bf16_t* residual, bf16_t* y, float* __restrict__ y_f32, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave / KW, part = wave % KW;
  const int n0 = (blockIdx.x * (4 / KW) + grp) * ROWS;
  const int kq = ((K / 32 + KW - 1) / KW) * 32;        // elements per wave (whole blocks)
  const int k_lo = part * kq, k_hi = min(K, k_lo + kq);
  const fp4x2_t* wr[ROWS];
  const e8m0_t* sr[ROWS];
  float acc[ROWS];
  bf16_t epi_raw[ROWS], bia_raw[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    acc[r] = 0.f;
    // epilogue operands requested up front, branch-free (null -> x[0]); their latency hides under the weight stream
    const int n = min(n0 + r, N - 1);
    wr[r] = W + (size_t)n * ldw;
    sr[r] = S + (size_t)n * (K >> 5);
    epi_raw[r] = (residual ? residual : x)[residual ? n : 0];
    bia_raw[r] = (bias ? bias : x)[bias ? n : 0];
  }
  for (int base = k_lo; base < k_hi; base += PRE * 2048) {
    u32x4_t xv[PRE][4], wv[PRE][ROWS];
    unsigned sv[PRE][ROWS];
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 2048 + lane * 32;
      const int cc = c < k_hi ? c : k_lo;                    // clamped (valid) address; its product is masked out
#pragma unroll
      for (int i = 0; i < 4; ++i) xv[it][i] = *reinterpret_cast<const u32x4_t*>(x + cc + 8 * i);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        wv[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + (cc >> 1)));
        sv[it][r] = sr[r][cc >> 5];
      }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const bool in = base + it * 2048 + lane * 32 < k_hi;
      float s[ROWS];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) s[r] = e8m0_f32(sv[it][r]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float lo[8], hi[8], xf[16];
        unpack8(xv[it][2 * h], lo);
        unpack8(xv[it][2 * h + 1], hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          xf[i] = in ? lo[i] : 0.f;
          xf[8 + i] = in ? hi[i] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[r] = dot16_fp4(wv[it][r][2 * h], wv[it][r][2 * h + 1], s[r], xf, acc[r]);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < ROWS; ++r) acc[r] = wave_sum(acc[r]);
  if (KW > 1) {
    __shared__ float partial[4][ROWS];
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < ROWS; ++r) partial[wave][r] = acc[r];
    }
    __syncthreads();
    if (part != 0) return;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      float s = partial[wave][r];
#pragma unroll
      for (int p = 1; p < KW; ++p) s += partial[wave + p][r];
      acc[r] = s;
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = n0 + r;
      if (n >= N) break;
      float v = rbf(acc[r] + (bias ? bf2f(bia_raw[r]) : 0.f));
      if (residual) v = rbf(v + bf2f(epi_raw[r]));
      if (y) y[n] = f2bf(v);
      if (y_f32) y_f32[n] = v;
    }
  }
}

// ---------------------------------------------------------------- dequantisation (prefill scratch layer)
// dst[32 i .. 32 i + 32) = bf16(code * 2^e_i): exact.  One block per thread: one 16-B load, one scale byte, four 16-B stores.
__global__ __launch_bounds__(256) void dequant_fp4_kernel(const fp4x2_t* __restrict__ src, const e8m0_t* __restrict__ scale,
                                                          bf16_t* __restrict__ dst, long long n32) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n32; i += (long long)gridDim.x * 256) {
    const float s = e8m0_f32(scale[i]);
    const u32x4_t w = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(src) + i);
    u32x4_t* d = reinterpret_cast<u32x4_t*>(dst) + 4 * i;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float f[8];
      const f32x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[j], s, 0);
      const f32x2_t b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[j], s, 1);
      const f32x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[j], s, 2);
      const f32x2_t e = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w[j], s, 3);
      f[0] = a[0]; f[1] = a[1]; f[2] = b[0]; f[3] = b[1]; f[4] = c[0]; f[5] = c[1]; f[6] = e[0]; f[7] = e[1];
      d[j] = pack8(f);
    }
  }
}

// ================================================================ launchers
// codes: K / 2 bytes per row at a 16-B aligned stride; scales: K / 32 bytes per row, contiguous
static inline bool fp4_k_ok(int K, int ldw) { return K > 0 && K % 32 == 0 && ldw >= K / 2 && ldw % 16 == 0; }

// (PRE, XC) by row length: PRE K-steps of 2048 codes pre-issued per batch (the whole row up to K = 4096), XC 2048-element chunks of x
#define DEC4_DISPATCH(KERNEL, ROWS, K, ...)                                 \
  do {                                                                      \
    if ((K) <= 2048) KERNEL<ROWS, 1, 1> __VA_ARGS__;                        \
    else if ((K) <= 4096) KERNEL<ROWS, 2, 2> __VA_ARGS__;                   \
    else KERNEL<ROWS, 2, 4> __VA_ARGS__;                                    \
  } while (0)

#ifndef QKV4_ROWS
#define QKV4_ROWS 1               // rows per wave: 39 / 51 VGPRs (PRE 1 / 2), 8 waves per SIMD; two rows cost 103 / 120 VGPRs and half the waves
#endif
extern "C" int svlm_dec_qkv_fp4(const void* x, const void* ln_w, float eps, const void* W4, int ldw, const void* w_scale, const void* bias,
                                void* q_out, void* k_planes, void* v_planes, const int* slot_of, const int* len_dev, int len_host, int K, int qd,
                                int kd, int D, int n_slots, void* k_lin, void* v_lin, int lin_rows, void* stream) {
  SVLM_CHECK_ARG(fp4_k_ok(K, ldw) && K <= 8192 && w_scale != nullptr, "svlm_dec_qkv_fp4: bad K=%d (a multiple of 32) ldw=%d or no scales", K, ldw);
  if (!dec_qkv_args_ok("svlm_dec_qkv_fp4", "svlm_dec_qkv_fp4", qd, kd, D, n_slots, bias, k_lin, v_lin, lin_rows, len_dev, len_host))
    return SVLM_EINVAL;
  const int N = qd + 2 * kd;
  DEC4_DISPATCH(dec_qkv_fp4_kernel, QKV4_ROWS, K, <<<(N + 4 * QKV4_ROWS - 1) / (4 * QKV4_ROWS), 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const fp4x2_t*)W4, ldw, (const e8m0_t*)w_scale, (const bf16_t*)bias, (bf16_t*)q_out,
      (bf16_t*)k_planes, (bf16_t*)v_planes, slot_of, len_dev, len_host, N, K, qd, kd, D, n_slots, (bf16_t*)k_lin, (bf16_t*)v_lin, lin_rows));
  return svlm_check_launch("svlm_dec_qkv_fp4");
}

#ifndef GU4_ROWS
#define GU4_ROWS 1                // gate rows (and as many up rows) per wave: 66 / 73 VGPRs (PRE 1 / 2), 7 / 6 waves per SIMD; 2: 118 / 155 VGPRs
#endif
extern "C" int svlm_dec_gate_up_fp4(const void* x, const void* ln_w, float eps, const void* W4, int ldw, const void* w_scale, void* h, int I,
                                    int K, void* stream) {
  SVLM_CHECK_ARG(fp4_k_ok(K, ldw) && K <= 8192 && I > 0 && w_scale != nullptr, "svlm_dec_gate_up_fp4: bad I=%d K=%d ldw=%d", I, K, ldw);
  DEC4_DISPATCH(dec_gate_up_fp4_kernel, GU4_ROWS, K, <<<(I + 4 * GU4_ROWS - 1) / (4 * GU4_ROWS), 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const fp4x2_t*)W4, ldw, (const e8m0_t*)w_scale, (bf16_t*)h, I, K));
  return svlm_check_launch("svlm_dec_gate_up_fp4");
}

extern "C" int svlm_gemv_fp4(const void* x, const void* W4, int ldw, const void* w_scale, const void* bias, const void* residual, void* y,
                             float* y_f32, int N, int K, int act, void* stream) {
  SVLM_CHECK_ARG(N > 0 && fp4_k_ok(K, ldw) && w_scale != nullptr, "svlm_gemv_fp4: bad shape N=%d K=%d (a multiple of 32) ldw=%d or no scales",
                 N, K, ldw);
  SVLM_CHECK_ARG(act == SVLM_ACT_NONE, "svlm_gemv_fp4: activation %d not supported (ACT_NONE only)", act);
  SVLM_CHECK_ARG(y || y_f32, "svlm_gemv_fp4: no output buffer");
  hipStream_t s = (hipStream_t)stream;
  const bf16_t *xb = (const bf16_t*)x, *bb = (const bf16_t*)bias, *rb = (const bf16_t*)residual;
  const fp4x2_t* w = (const fp4x2_t*)W4;
  const e8m0_t* sc = (const e8m0_t*)w_scale;
  bf16_t* yb = (bf16_t*)y;
  // the K-split choice of svlm_gemv_fp8: a skinny output with a long reduction (down_proj) splits K over the workgroup's waves
  if (N <= 8192 && K >= 4096) {
    gemv_fp4_kernel<2, 4, 2><<<(N + 1) / 2, 256, 0, s>>>(xb, w, ldw, sc, bb, rb, yb, y_f32, N, K);
  } else if (N >= 4096 || (long long)N * K >= (8LL << 20)) {
    if (K <= 2048) gemv_fp4_kernel<2, 1, 1><<<(N + 7) / 8, 256, 0, s>>>(xb, w, ldw, sc, bb, rb, yb, y_f32, N, K);
    else gemv_fp4_kernel<2, 1, 2><<<(N + 7) / 8, 256, 0, s>>>(xb, w, ldw, sc, bb, rb, yb, y_f32, N, K);
  } else {
    if (K <= 2048) gemv_fp4_kernel<1, 1, 1><<<(N + 3) / 4, 256, 0, s>>>(xb, w, ldw, sc, bb, rb, yb, y_f32, N, K);
    else gemv_fp4_kernel<1, 1, 2><<<(N + 3) / 4, 256, 0, s>>>(xb, w, ldw, sc, bb, rb, yb, y_f32, N, K);
  }
  return svlm_check_launch("svlm_gemv_fp4");
}

extern "C" int svlm_dequant_fp4_bf16(const void* src4, const void* scale, void* dst, int rows, int cols, void* stream) {
  SVLM_CHECK_ARG(rows > 0 && cols > 0 && cols % 32 == 0 && src4 && scale && dst, "svlm_dequant_fp4_bf16: bad rows=%d cols=%d", rows, cols);
  const long long n32 = (long long)rows * (cols / 32);
  const long long want = (n32 + 255) / 256;
  const int grid = (int)(want < 8192 ? want : 8192);
  dequant_fp4_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const fp4x2_t*)src4, (const e8m0_t*)scale, (bf16_t*)dst, n32);
  return svlm_check_launch("svlm_dequant_fp4_bf16");
}
