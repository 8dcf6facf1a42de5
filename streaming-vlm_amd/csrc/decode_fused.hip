// Fused decode-step (T = 1) kernels: the small per-layer ops around each weight-streaming GEMV are
// folded into its prologue / epilogue, because at batch 1 every separate launch costs ~4-5 us of
// dependent memory latency while the work it does is nanoseconds.
//
//   svlm_dec_qkv       RMSNorm(x) -> [q|k|v] = W x + b -> q to a buffer, k and v STRAIGHT into the
//                      KV pool slot of the new token (un-rotated)
//                      (qwen2/language_forward.py:183,80-82 + StreamingCache.update, streaming_cache.py:72-73)
//   svlm_dec_gate_up   RMSNorm(x) -> h = silu(Wg x) * (Wu x)            (Qwen2MLP, language_forward.py:200-201)
//   svlm_dec_lm_head   final RMSNorm -> last-row logits (fp32 copy of the bf16 value) -> repetition penalty /
//                      EOS suppression -> per-workgroup argmax candidates   (language_forward.py:315,
//                      model_forward.py:243, streaming_generate_qwen.py:73-99)
//   svlm_argmax_finish winner over the candidates + device-side token feedback
// The o_proj and down_proj GEMVs keep using svlm_gemv_bf16 with its residual epilogue.
//
// All are HBM-bound weight streams: 16-B loads straight to VGPRs, the normalised activation row is
// staged once per workgroup in LDS (bf16, rounded exactly where the eager module rounds).
//
// This file holds the bf16 K loop (fma_batch, wave_dots), the kernels' names and the launchers.  What surrounds the K loop is the
// shell of each op in dec_shell.h, shared with the e4m3 (decode_fp8.hip) and MXFP4 (decode_fp4.hip) kernels through a weight-format
// policy (WBf16, dec_stream.h); the KV append, the candidate scoring and the candidate reduce are in dec_epi.h.
#include "common.h"
#include "dec_xrow.h"
#include "dec_stream.h"
#include "dec_launch.h"           // host side: lane-count switch, qkv argument checks
#include "dec_shell.h"            // the kernel shells over WBf16 (dec_stream.h); epilogue pieces: dec_epi.h

template <int NR, int PRE>
__device__ __forceinline__ void fma_batch(const WPre<NR, PRE>& pre, const bf16_t* xs, int base, int K, float (&acc)[NR]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 512 + lane * 8;
    float xf[8];
    unpack8(*reinterpret_cast<const u32x4_t*>(xs + (c < K ? c : 0)), xf);
    if (c >= K) {
#pragma unroll
      for (int i = 0; i < 8; ++i) xf[i] = 0.f;
    }
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      float wf[8];
      unpack8(pre.w[it][r], wf);
#pragma unroll
      for (int i = 0; i < 8; ++i) acc[r] = fmaf(wf[i], xf[i], acc[r]);
    }
  }
}

// acc[r] = W[row[r]] . xs   for NR rows of one wave; `pre` holds K-steps [0, PRE) already in flight
template <int NR, int PRE>
__device__ __forceinline__ void wave_dots(const bf16_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NR], WPre<NR, PRE>& pre) {
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = 0.f;
  fma_batch<NR, PRE>(pre, xs, 0, K, acc);
  for (int base = PRE * 512; base < K; base += PRE * 512) {
    preload_w<NR, PRE>(wr, base, K, pre);
    __builtin_amdgcn_sched_barrier(0);                       // every load of the batch is issued before its first FMA
    fma_batch<NR, PRE>(pre, xs, base, K, acc);
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) acc[r] = wave_sum(acc[r]);
}

// ---------------------------------------------------------------- QKV + KV append
template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_qkv_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                      const bf16_t* __restrict__ W, int ldw, const bf16_t* __restrict__ bias,
                                                      bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_planes,
                                                      bf16_t* __restrict__ v_planes, const int* __restrict__ slot_of,
                                                      const int* __restrict__ len_dev, int len_host, int N, int K, int qd, int kd,
                                                      int D, int n_slots, bf16_t* __restrict__ k_lin, bf16_t* __restrict__ v_lin,
                                                      int lin_rows) {
  dec_qkv_body<WBf16, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, /* S: none */ nullptr, bias, q_out, k_planes, v_planes, slot_of, len_dev, len_host, N, K, qd, kd, D,
                                     n_slots, k_lin, v_lin, lin_rows);
}

// ---------------------------------------------------------------- gate/up + SwiGLU
template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_gate_up_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                          const bf16_t* __restrict__ W, int ldw, bf16_t* __restrict__ h, int I, int K) {
  dec_gate_up_body<WBf16, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, /* S: none */ nullptr, h, I, K);
}

// ---------------------------------------------------------------- lm_head + penalty + argmax candidates
template <int ROWS, int PRE, int XC>
__global__ __launch_bounds__(256) void dec_lm_head_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                          const bf16_t* __restrict__ W, int ldw, float* __restrict__ logits,
                                                          const unsigned char* __restrict__ seen, float penalty,
                                                          const int* __restrict__ suppress, int n_suppress,
                                                          float* __restrict__ part_val, int* __restrict__ part_idx, int V, int K,
                                                          float inv_temp, const unsigned* __restrict__ rng,
                                                          const int* __restrict__ state) {
  dec_lm_head_body<WBf16, ROWS, PRE, XC>(x, ln_w, eps, W, ldw, /* S: none */ nullptr, logits, seen, penalty, suppress, n_suppress, part_val, part_idx, V, K,
                                         inv_temp, rng, state);
}

__global__ __launch_bounds__(1024) void argmax_finish_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                             int n_parts, unsigned char* seen, int* tok_buf, int* state, int advance_kv) {
  argmax_finish_body(part_val, part_idx, n_parts, seen, tok_buf, state, advance_kv);
}

// ================================================================ launchers
static inline bool smem_ok(int K) { return K > 0 && K % 8 == 0 && K <= 8192; }

// (PRE, XC) by row length: the whole row in one pre-issued batch at K <= 1536, batches of 4 K-steps beyond;
// one 2048-element chunk of x per thread-pass
#define DEC_DISPATCH(KERNEL, ROWS, K, ...)                                  \
  do {                                                                      \
    if ((K) <= 1536) KERNEL<ROWS, 3, 1> __VA_ARGS__;                        \
    else if ((K) <= 2048) KERNEL<ROWS, 4, 1> __VA_ARGS__;                   \
    else if ((K) <= 4096) KERNEL<ROWS, 4, 2> __VA_ARGS__;                   \
    else KERNEL<ROWS, 4, 4> __VA_ARGS__;                                    \
  } while (0)

extern "C" int svlm_dec_qkv_lin(const void* x, const void* ln_w, float eps, const void* W, int ldw, const void* bias, void* q_out,
                                void* k_planes, void* v_planes, const int* slot_of, const int* len_dev, int len_host, int K, int qd,
                                int kd, int D, int n_slots, void* k_lin, void* v_lin, int lin_rows, void* stream);
extern "C" int svlm_dec_qkv(const void* x, const void* ln_w, float eps, const void* W, int ldw, const void* bias, void* q_out,
                            void* k_planes, void* v_planes, const int* slot_of, const int* len_dev, int len_host, int K, int qd,
                            int kd, int D, int n_slots, void* stream) {
  return svlm_dec_qkv_lin(x, ln_w, eps, W, ldw, bias, q_out, k_planes, v_planes, slot_of, len_dev, len_host, K, qd, kd, D, n_slots, nullptr, nullptr,
                          0, stream);
}

// k_lin / v_lin (optional, together): the layer's linear planes of lin_rows rows (svlm_decode_attn_lin); the new token's K row goes there
// too, UN-rotated, at its logical row, and its V row as it is.
extern "C" int svlm_dec_qkv_lin(const void* x, const void* ln_w, float eps, const void* W, int ldw, const void* bias, void* q_out,
                                void* k_planes, void* v_planes, const int* slot_of, const int* len_dev, int len_host, int K, int qd,
                                int kd, int D, int n_slots, void* k_lin, void* v_lin, int lin_rows, void* stream) {
  SVLM_CHECK_ARG(smem_ok(K) && ldw >= K && ldw % 8 == 0, "svlm_dec_qkv: bad K=%d ldw=%d", K, ldw);
  if (!dec_qkv_args_ok("svlm_dec_qkv", "svlm_dec_qkv_lin", qd, kd, D, n_slots, bias, k_lin, v_lin, lin_rows, len_dev, len_host))
    return SVLM_EINVAL;
  const int N = qd + 2 * kd;
  // one row per wave: two rows per wave were measured on the 7B shape (4608 x 3584) and are slower (9.96 vs 8.8 us)
  DEC_DISPATCH(dec_qkv_kernel, 1, K, <<<(N + 3) / 4, 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, (const bf16_t*)bias, (bf16_t*)q_out, (bf16_t*)k_planes,
      (bf16_t*)v_planes, slot_of, len_dev, len_host, N, K, qd, kd, D, n_slots, (bf16_t*)k_lin, (bf16_t*)v_lin, lin_rows));
  return svlm_check_launch("svlm_dec_qkv");
}

extern "C" int svlm_dec_gate_up(const void* x, const void* ln_w, float eps, const void* W, int ldw, void* h, int I, int K, void* stream) {
  SVLM_CHECK_ARG(smem_ok(K) && ldw >= K && ldw % 8 == 0 && I > 0, "svlm_dec_gate_up: bad I=%d K=%d ldw=%d", I, K, ldw);
#ifndef GU_ROWS
#define GU_ROWS 1                 // gate rows (and as many up rows) per wave: 1 measured against 2 on MI355X -- 2B 10.83 -> 10.43 us, 7B 44.0 -> 42.8 us
#endif
  DEC_DISPATCH(dec_gate_up_kernel, GU_ROWS, K, <<<(I + 4 * GU_ROWS - 1) / (4 * GU_ROWS), 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, (bf16_t*)h, I, K));
  return svlm_check_launch("svlm_dec_gate_up");
}

#ifndef LM_ROWS
#define LM_ROWS 2                 // vocabulary rows per wave: 2 measured against 4 (2B: 78.8 -> 75.7 us; 7B unchanged) and 1 / 3 / 8
#endif
extern "C" long long svlm_dec_lm_head_ws_bytes(int V) { return V <= 0 ? SVLM_EINVAL : (long long)((V + 4 * LM_ROWS - 1) / (4 * LM_ROWS)) * 8; }

static int dec_lm_head_launch(const void* x, const void* ln_w, float eps, const void* W, int ldw, float* logits, const void* seen,
                              float penalty, const int* suppress, int n_suppress, void* ws, int V, int K, float inv_temp,
                              const unsigned* rng, const int* state, void* stream) {
  SVLM_CHECK_ARG(smem_ok(K) && ldw >= K && ldw % 8 == 0 && V > 0, "svlm_dec_lm_head: bad V=%d K=%d ldw=%d", V, K, ldw);
  SVLM_CHECK_ARG(penalty > 0.f && n_suppress >= 0 && n_suppress <= 8 && ws != nullptr && logits != nullptr, "svlm_dec_lm_head: bad sampling args");
  const int nb = (V + 4 * LM_ROWS - 1) / (4 * LM_ROWS);
  float* pv = (float*)ws;
  int* pi = (int*)(pv + nb);
  DEC_DISPATCH(dec_lm_head_kernel, LM_ROWS, K, <<<nb, 256, K * 2, (hipStream_t)stream>>>(
      (const bf16_t*)x, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, logits, (const unsigned char*)seen, penalty, suppress,
      n_suppress, pv, pi, V, K, inv_temp, rng, state));
  return svlm_check_launch("svlm_dec_lm_head");
}

extern "C" int svlm_dec_lm_head(const void* x, const void* ln_w, float eps, const void* W, int ldw, float* logits, const void* seen,
                                float penalty, const int* suppress, int n_suppress, void* ws, int V, int K, void* stream) {
  return dec_lm_head_launch(x, ln_w, eps, W, ldw, logits, seen, penalty, suppress, n_suppress, ws, V, K, 1.0f, nullptr, nullptr, stream);
}

// The same launch with temperature sampling folded in: the candidates are argmax(score / T + Gumbel noise), an exact draw from
// softmax(score / T) (sampling.hip); rng = {seed lo, seed hi} and state = {kv_len, cur} live in device memory.
extern "C" int svlm_dec_lm_head_sample(const void* x, const void* ln_w, float eps, const void* W, int ldw, float* logits, const void* seen,
                                       float penalty, const int* suppress, int n_suppress, void* ws, int V, int K, float temperature,
                                       const unsigned* rng, const int* state, void* stream) {
  SVLM_CHECK_ARG(temperature > 0.f && rng != nullptr && state != nullptr, "svlm_dec_lm_head_sample: bad temperature=%f / null rng or state", temperature);
  return dec_lm_head_launch(x, ln_w, eps, W, ldw, logits, seen, penalty, suppress, n_suppress, ws, V, K, 1.0f / temperature, rng, state, stream);
}

extern "C" int svlm_argmax_finish(const void* ws, int V, void* seen, int* tok_buf, int* state, int advance_kv, void* stream) {
  SVLM_CHECK_ARG(V > 0 && ws != nullptr, "svlm_argmax_finish: bad args");
  const int nb = (V + 4 * LM_ROWS - 1) / (4 * LM_ROWS);
  const float* pv = (const float*)ws;
  const int* pi = (const int*)(pv + nb);
  argmax_finish_kernel<<<1, 1024, 0, (hipStream_t)stream>>>(pv, pi, nb, (unsigned char*)seen, tok_buf, state, advance_kv);
  return svlm_check_launch("svlm_argmax_finish");
}
