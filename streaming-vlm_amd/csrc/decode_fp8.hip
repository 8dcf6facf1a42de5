// Decode-step (T = 1) weight-streaming GEMVs on OCP e4m3 weights with one power-of-two scale per output row (the opt-in
// `llm_fp8` engine, weights.py:quantize_rows_fp8_pow2).  The fused kernels are the SHELLS of the bf16 ones (dec_shell.h) over the
// policy WFp8 (dec_fp8.h) -- one prologue, one epilogue (dec_epi.h), the same rounding points -- around this file's K loop (fma_batch8,
// wave_dots8); the plain GEMV and the dequantisation are this file's own.  Entry, its bf16 counterpart:
//
//   svlm_dec_qkv_fp8              svlm_dec_qkv_lin      (decode_fused.hip)  RMSNorm -> QKV + bias -> K/V append (+ linear planes)
//   svlm_dec_gate_up_fp8          svlm_dec_gate_up      (decode_fused.hip)  RMSNorm -> gate/up -> SwiGLU
//   svlm_gemv_fp8                 svlm_gemv_bf16        (gemv.hip)          o_proj / down_proj + residual, prefill's last-row logits
//   svlm_dec_lm_head[_sample]_fp8 svlm_dec_lm_head[_sample]                 final RMSNorm -> logits -> penalty -> argmax candidates
//   svlm_dequant_fp8_bf16         (none)                                    q * s -> bf16, the prefill's scratch layer
//
// With s a power of two, q * s is exact in bf16 (W') and every product q * x is exact in fp32, so sum_k(q_k x_k) * s is the bf16
// GEMV on W' up to the fp32 summation order: the scale is applied once per row, in the epilogue, where it is exact too.
//
// Structure (the bf16 kernels' measurements carry over): one 16-B load carries 16 weights and goes straight to VGPRs, every load
// of a batch is issued before the first FMA, the normalised activation row is staged in LDS behind LDS-only barriers.  A lane owns
// 16 consecutive K elements per K-step, a K-step is 1024 elements.  Conversion: v_cvt_pk_f32_fp8 (two codes -> two fp32, exact,
// subnormals included) feeding the same fp32 FMAs the bf16 path sums with.
#include "common.h"
#include "dec_xrow.h"
#include "dec_fp8.h"              // x16, dot16, W8Pre, preload_w8, the policy WFp8: shared with decode_batch_fp8.hip
#include "dec_launch.h"           // host side: lane-count switch, qkv argument checks
#include "dec_shell.h"            // the kernel shells over WFp8; epilogue pieces: dec_epi.h

// ---------------------------------------------------------------- fused decode kernels (x staged in LDS)
template <int NR, int PRE>
__device__ __forceinline__ void fma_batch8(const W8Pre<NR, PRE>& pre, const bf16_t* xs, int base, int K, float (&acc)[NR]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    float xf[16];
    x16(xs, base + it * 1024 + lane * 16, K, xf);
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[r] = dot16(pre.w[it][r], xf, acc[r]);
  }
}

// acc[r] = sum_k q[row r][k] * xs[k] for NR rows of one wave (unscaled); `pre` holds K-steps [0, PRE) already in flight
template <int NR, int PRE>
__device__ __forceinline__ void wave_dots8(const fp8_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NR], W8Pre<NR, PRE>& pre) {
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.f;
  fma_batch8<NR, PRE>(pre, xs, 0, K, acc);
  for (int base = PRE * 1024; base < K; base += PRE * 1024) {
    preload_w8<NR, PRE>(wr, base, K, pre);
    __builtin_amdgcn_sched_barrier(0);                       // every load of the batch is issued before its first FMA
    fma_batch8<NR, PRE>(pre, xs, base, K, acc);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = wave_sum(acc[r]);
}

template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_qkv_fp8_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                          const fp8_t* __restrict__ W, int ldw, const float* __restrict__ w_scale,
                                                          const bf16_t* __restrict__ bias, bf16_t* __restrict__ q_out,
                                                          bf16_t* __restrict__ k_planes, bf16_t* __restrict__ v_planes,
                                                          const int* __restrict__ slot_of, const int* __restrict__ len_dev, int len_host,
                                                          int N, int K, int qd, int kd, int D, int n_slots, bf16_t* __restrict__ k_lin,
                                                          bf16_t* __restrict__ v_lin, int lin_rows) {
  dec_qkv_body<WFp8, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, w_scale, bias, q_out, k_planes, v_planes, slot_of, len_dev, len_host, N, K, qd, kd, D,
                                    n_slots, k_lin, v_lin, lin_rows);
}

template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_gate_up_fp8_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                              const fp8_t* __restrict__ W, int ldw, const float* __restrict__ w_scale,
                                                              bf16_t* __restrict__ h, int I, int K) {
  dec_gate_up_body<WFp8, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, w_scale, h, I, K);
}

template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_lm_head_fp8_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                              const fp8_t* __restrict__ W, int ldw, const float* __restrict__ w_scale,
                                                              float* __restrict__ logits, const unsigned char* __restrict__ seen,
                                                              float penalty, const int* __restrict__ suppress, int n_suppress,
                                                              float* __restrict__ part_val, int* __restrict__ part_idx, int V, int K,
                                                              float inv_temp, const unsigned* __restrict__ rng,
                                                              const int* __restrict__ state) {
  dec_lm_head_body<WFp8, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, w_scale, logits, seen, penalty, suppress, n_suppress, part_val, part_idx, V, K,
                                        inv_temp, rng, state);
}

// ---------------------------------------------------------------- plain GEMV (x from global), optional K split over the waves
// The 4 waves of a workgroup form 4 / KW groups of ROWS rows each; the KW waves of a group take one 1/KW share of K each
// (KW = 4: the long-K form of svlm_gemv_bf16, for a skinny output with a long reduction).
template <int ROWS, int KW, int PRE>
__global__ __launch_bounds__(256) void gemv_fp8_kernel(const bf16_t* __restrict__ x, const fp8_t* __restrict__ W, int ldw,
                                                       const float* __restrict__ w_scale, const bf16_t* __restrict__ bias,
                                                       const bf16_t* residual, bf16_t* y, float* __restrict__ y_f32, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave / KW, part = wave % KW;
  const int n0 = (blockIdx.x * (4 / KW) + grp) * ROWS;
  const int kq = ((K / 16 + KW - 1) / KW) * 16;        // elements per wave (multiple of 16)
  const int k_lo = part * kq, k_hi = min(K, k_lo + kq);
  const fp8_t* wr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wr[r] = W + (size_t)min(n0 + r, N - 1) * ldw;
  float acc[ROWS];
  bf16_t epi_raw[ROWS], bia_raw[ROWS];
  float spre[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    acc[r] = 0.f;
    // epilogue operands requested up front, branch-free (null -> x[0]); their latency hides under the weight stream
    const int n = min(n0 + r, N - 1);
    epi_raw[r] = (residual ? residual : x)[residual ? n : 0];
    bia_raw[r] = (bias ? bias : x)[bias ? n : 0];
    spre[r] = w_scale[n];
  }
  for (int base = k_lo; base < k_hi; base += PRE * 1024) {
    u32x4_t xa[PRE], xb[PRE], wv[PRE][ROWS];
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 1024 + lane * 16;
      const int cc = c < k_hi ? c : k_lo;
      xa[it] = *reinterpret_cast<const u32x4_t*>(x + cc);
      xb[it] = *reinterpret_cast<const u32x4_t*>(x + cc + 8);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) wv[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + cc));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const bool in = base + it * 1024 + lane * 16 < k_hi;
      float lo[8], hi[8], xf[16];
      unpack8(xa[it], lo);
      unpack8(xb[it], hi);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        xf[i] = in ? lo[i] : 0.f;
        xf[8 + i] = in ? hi[i] : 0.f;
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) acc[r] = dot16(wv[it][r], xf, acc[r]);
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
      float v = rbf(acc[r] * spre[r] + (bias ? bf2f(bia_raw[r]) : 0.f));
      if (residual) v = rbf(v + bf2f(epi_raw[r]));
      if (y) y[n] = f2bf(v);
      if (y_f32) y_f32[n] = v;
    }
  }
}

// ---------------------------------------------------------------- dequantisation (prefill scratch layer)
// dst[r, c] = bf16(q[r, c] * s[r]): exact for power-of-two scales.  16 codes per thread: one 16-B load, two 16-B stores.
__global__ __launch_bounds__(256) void dequant_fp8_kernel(const fp8_t* __restrict__ src, const float* __restrict__ scale,
                                                          bf16_t* __restrict__ dst, long long n16, int cols16) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n16; i += (long long)gridDim.x * 256) {
    const float s = scale[i / cols16];
    const u32x4_t w = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(src) + i);
    float f[16];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], false);
      const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[j], true);
      f[4 * j] = lo[0] * s;
      f[4 * j + 1] = lo[1] * s;
      f[4 * j + 2] = hi[0] * s;
      f[4 * j + 3] = hi[1] * s;
    }
    float a[8], b[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { a[j] = f[j]; b[j] = f[8 + j]; }
    u32x4_t* d = reinterpret_cast<u32x4_t*>(dst) + 2 * i;
    d[0] = pack8(a);
    d[1] = pack8(b);
  }
}

// ================================================================ launchers
static inline bool fp8_k_ok(int K, int ldw) { return K > 0 && K % 16 == 0 && K <= 8192 && ldw >= K && ldw % 16 == 0; }

// (PRE, XC) by row length: PRE K-steps of 1024 codes pre-issued per batch (the whole row up to K = 4096), XC 2048-element chunks of x
#define DEC8_DISPATCH(KERNEL, ROWS, K, ...)                                 \
  do {                                                                      \
    if ((K) <= 1024) KERNEL<ROWS, 1, 1> __VA_ARGS__;                        \
    else if ((K) <= 2048) KERNEL<ROWS, 2, 1> __VA_ARGS__;                   \
    else if ((K) <= 4096) KERNEL<ROWS, 4, 2> __VA_ARGS__;                   \
    else KERNEL<ROWS, 4, 4> __VA_ARGS__;                                    \
  } while (0)

#ifndef QKV8_ROWS
#define QKV8_ROWS 1               // rows per wave: 1 measured against 2 on MI355X (cold, 8 layers) -- 2B 4.84 vs 5.14 us, 7B 8.13 vs 8.44 us
#endif
extern "C" int svlm_dec_qkv_fp8(const void* x, const void* ln_w, float eps, const void* W8, int ldw, const float* w_scale, const void* bias,
                                void* q_out, void* k_planes, void* v_planes, const int* slot_of, const int* len_dev, int len_host, int K, int qd,
                                int kd, int D, int n_slots, void* k_lin, void* v_lin, int lin_rows, void* stream) {
  SVLM_CHECK_ARG(fp8_k_ok(K, ldw) && w_scale != nullptr, "svlm_dec_qkv_fp8: bad K=%d ldw=%d (multiples of 16) or no scales", K, ldw);
  if (!dec_qkv_args_ok("svlm_dec_qkv_fp8", "svlm_dec_qkv_fp8", qd, kd, D, n_slots, bias, k_lin, v_lin, lin_rows, len_dev, len_host))
    return SVLM_EINVAL;
  const int N = qd + 2 * kd;
  DEC8_DISPATCH(dec_qkv_fp8_kernel, QKV8_ROWS, K, <<<(N + 4 * QKV8_ROWS - 1) / (4 * QKV8_ROWS), 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale, (const bf16_t*)bias, (bf16_t*)q_out, (bf16_t*)k_planes,
      (bf16_t*)v_planes, slot_of, len_dev, len_host, N, K, qd, kd, D, n_slots, (bf16_t*)k_lin, (bf16_t*)v_lin, lin_rows));
  return svlm_check_launch("svlm_dec_qkv_fp8");
}

#ifndef GU8_ROWS
#define GU8_ROWS 1                // gate rows (and as many up rows) per wave: 1 measured against 2 -- 2B 9.18 vs 8.97 us, 7B 24.98 vs 26.36 us
#endif
extern "C" int svlm_dec_gate_up_fp8(const void* x, const void* ln_w, float eps, const void* W8, int ldw, const float* w_scale, void* h, int I,
                                    int K, void* stream) {
  SVLM_CHECK_ARG(fp8_k_ok(K, ldw) && I > 0 && w_scale != nullptr, "svlm_dec_gate_up_fp8: bad I=%d K=%d ldw=%d", I, K, ldw);
  DEC8_DISPATCH(dec_gate_up_fp8_kernel, GU8_ROWS, K, <<<(I + 4 * GU8_ROWS - 1) / (4 * GU8_ROWS), 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale, (bf16_t*)h, I, K));
  return svlm_check_launch("svlm_dec_gate_up_fp8");
}

// the candidates' layout of svlm_dec_lm_head (two vocabulary rows per wave, one candidate per workgroup), so that
// svlm_argmax_finish and svlm_dec_lm_head_ws_bytes serve both
#define LM8_ROWS 2
static int dec_lm_head_fp8_launch(const void* x, const void* ln_w, float eps, const void* W8, int ldw, const float* w_scale, float* logits,
                                  const void* seen, float penalty, const int* suppress, int n_suppress, void* ws, int V, int K, float inv_temp,
                                  const unsigned* rng, const int* state, void* stream) {
  SVLM_CHECK_ARG(fp8_k_ok(K, ldw) && V > 0 && w_scale != nullptr, "svlm_dec_lm_head_fp8: bad V=%d K=%d ldw=%d", V, K, ldw);
  SVLM_CHECK_ARG(penalty > 0.f && n_suppress >= 0 && n_suppress <= 8 && ws != nullptr && logits != nullptr, "svlm_dec_lm_head_fp8: bad sampling args");
  const int nb = (V + 4 * LM8_ROWS - 1) / (4 * LM8_ROWS);
  float* pv = (float*)ws;
  int* pi = (int*)(pv + nb);
  DEC8_DISPATCH(dec_lm_head_fp8_kernel, LM8_ROWS, K, <<<nb, 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale, logits, (const unsigned char*)seen, penalty, suppress,
      n_suppress, pv, pi, V, K, inv_temp, rng, state));
  return svlm_check_launch("svlm_dec_lm_head_fp8");
}

extern "C" int svlm_dec_lm_head_fp8(const void* x, const void* ln_w, float eps, const void* W8, int ldw, const float* w_scale, float* logits,
                                    const void* seen, float penalty, const int* suppress, int n_suppress, void* ws, int V, int K, void* stream) {
  return dec_lm_head_fp8_launch(x, ln_w, eps, W8, ldw, w_scale, logits, seen, penalty, suppress, n_suppress, ws, V, K, 1.0f, nullptr, nullptr,
                                stream);
}

extern "C" int svlm_dec_lm_head_sample_fp8(const void* x, const void* ln_w, float eps, const void* W8, int ldw, const float* w_scale,
                                           float* logits, const void* seen, float penalty, const int* suppress, int n_suppress, void* ws, int V,
                                           int K, float temperature, const unsigned* rng, const int* state, void* stream) {
  SVLM_CHECK_ARG(temperature > 0.f && rng != nullptr && state != nullptr, "svlm_dec_lm_head_sample_fp8: bad temperature=%f / null rng or state",
                 temperature);
  return dec_lm_head_fp8_launch(x, ln_w, eps, W8, ldw, w_scale, logits, seen, penalty, suppress, n_suppress, ws, V, K, 1.0f / temperature, rng,
                                state, stream);
}

extern "C" int svlm_gemv_fp8(const void* x, const void* W8, int ldw, const float* w_scale, const void* bias, const void* residual, void* y,
                             float* y_f32, int N, int K, int act, void* stream) {
  SVLM_CHECK_ARG(N > 0 && K > 0 && K % 16 == 0 && ldw % 16 == 0 && ldw >= K && w_scale != nullptr,
                 "svlm_gemv_fp8: bad shape N=%d K=%d ldw=%d (multiples of 16) or no scales", N, K, ldw);
  SVLM_CHECK_ARG(act == SVLM_ACT_NONE, "svlm_gemv_fp8: activation %d not supported (ACT_NONE only)", act);
  SVLM_CHECK_ARG(y || y_f32, "svlm_gemv_fp8: no output buffer");
  hipStream_t s = (hipStream_t)stream;
  const bf16_t *xb = (const bf16_t*)x, *bb = (const bf16_t*)bias, *rb = (const bf16_t*)residual;
  const fp8_t* w = (const fp8_t*)W8;
  bf16_t* yb = (bf16_t*)y;
  // the K-split choice of svlm_gemv_bf16: a skinny output with a long reduction (down_proj) splits K over the workgroup's waves
  if (N <= 8192 && K >= 4096) {
    gemv_fp8_kernel<2, 4, 3><<<(N + 1) / 2, 256, 0, s>>>(xb, w, ldw, w_scale, bb, rb, yb, y_f32, N, K);
  } else if (N >= 16384) {
    gemv_fp8_kernel<4, 1, 2><<<(N + 15) / 16, 256, 0, s>>>(xb, w, ldw, w_scale, bb, rb, yb, y_f32, N, K);
  } else if (N >= 4096 || (long long)N * K >= (8LL << 20)) {
    gemv_fp8_kernel<2, 1, 2><<<(N + 7) / 8, 256, 0, s>>>(xb, w, ldw, w_scale, bb, rb, yb, y_f32, N, K);
  } else {
    gemv_fp8_kernel<1, 1, 4><<<(N + 3) / 4, 256, 0, s>>>(xb, w, ldw, w_scale, bb, rb, yb, y_f32, N, K);
  }
  return svlm_check_launch("svlm_gemv_fp8");
}

extern "C" int svlm_dequant_fp8_bf16(const void* src8, const float* scale, void* dst, int rows, int cols, void* stream) {
  SVLM_CHECK_ARG(rows > 0 && cols > 0 && cols % 16 == 0 && src8 && scale && dst, "svlm_dequant_fp8_bf16: bad rows=%d cols=%d", rows, cols);
  const long long n16 = (long long)rows * (cols / 16);
  const long long want = (n16 + 255) / 256;
  const int grid = (int)(want < 8192 ? want : 8192);
  dequant_fp8_kernel<<<grid, 256, 0, (hipStream_t)stream>>>((const fp8_t*)src8, scale, (bf16_t*)dst, n16, cols / 16);
  return svlm_check_launch("svlm_dequant_fp8_bf16");
}
