// Lane-batched decode-step kernels: B independent streams ("lanes", B = 1..4) take their decode step together, so that every
// weight byte is read ONCE and every launch boundary is paid ONCE for B tokens.
//
//   svlm_decb_embed          x[b] = embed[tok_buf_b[cur_b]]                                       (the step's embedding gather)
//   svlm_decb_qkv            batched svlm_dec_qkv_lin: RMSNorm + QKV + bias + KV append to each lane's own pool slot / linear planes
//   svlm_decb_gemv           batched svlm_gemv_bf16 with residual (o_proj, down_proj), K split over the workgroup's waves for the
//                            same shapes as the single-row entry
//   svlm_decb_gate_up        batched svlm_dec_gate_up
//   svlm_decb_lm_head        batched svlm_dec_lm_head (greedy: penalty, suppression, argmax candidates per lane)
//   svlm_decb_argmax_finish  batched svlm_argmax_finish, one workgroup per lane
//   svlm_decb_lm_head_sample svlm_decb_lm_head whose candidates carry the Gumbel noise of svlm_dec_lm_head_sample for the lanes that
//                            draw with a plain temperature (per-lane sampling records, struct svlm_lane_sample)
//   svlm_decb_sample_finish  one workgroup per lane: svlm_argmax_finish over the candidates (greedy, Gumbel) or the top-k / top-p
//                            draw of svlm_penalty_sample on the lane's own logits row (dec_sample.h)
//
// The fused kernels are the lane-batched shells of dec_shell.h over the policy WBf16 (dec_stream.h), shared with decode_batch_fp8.hip
// and decode_batch_fp4.hip, around this file's K loop (fma_batch_b, wave_dots_b); their epilogue pieces (KV append, candidate scoring and
// reduce, residual tail) are those of the single-row kernels, in dec_epi.h.  The residual GEMVs, the embedding gather and the finish
// kernels are this file's own.
//
// Each wave loads its weight rows once (the same 16-B non-temporal loads and PRE run-ahead as decode_fused.hip) and multiplies them
// with the NB activation rows of the group.  The fused kernels stage the NB normalised rows in LDS; svlm_decb_gemv reads its NB
// un-normalised rows straight from global memory like svlm_gemv_bf16 does (a down_proj row of 4 lanes is 150 KB: it does not fit a
// workgroup's LDS share, and the rows are L2-resident).
//
// ARITHMETIC ORDER IS KEPT PER LANE: for one (lane, output row) the FMA sequence over K, the wave_sum, the K-split reduction
// part[0] + part[1] + part[2] + part[3] and every bf16 rounding point are those of the single-row kernel (whose device functions are
// shared through dec_xrow.h / dec_stream.h), so every output is bitwise the single-row kernel's.  How many rows a wave takes does not
// enter a row's arithmetic; only svlm_decb_lm_head must keep the single-row kernel's 8 vocabulary rows per workgroup, because the
// candidates are per workgroup.
//
// Per-lane pointers come from the LANE TABLE (struct svlm_lane, include/svlm.h).  A lane is LIVE in a step iff
// state[1] + 1 < limit; a lane that is not live is skipped by every kernel: no KV row, no token, no state change.
#include "common.h"
#include "dec_xrow.h"
#include "dec_stream.h"
#include "dec_lanes.h"            // svlm_lane, lane_live, load_rows, stage_rows, DECB_SWITCH_NB: shared by all lane-batched files
#include "dec_launch.h"           // host side: lane-count switch, qkv argument checks
#include "dec_shell.h"            // the kernel shells over WBf16 (dec_stream.h); epilogue pieces: dec_epi.h
#include "dec_sample.h"

// acc[b][r] += W[row r] . xs[b] over the PRE K-steps held in `pre`; per (b, r) the same FMA sequence as fma_batch (decode_fused.hip)
template <int NB, int NR, int PRE>
__device__ __forceinline__ void fma_batch_b(const WPre<NR, PRE>& pre, const bf16_t* xs, int base, int K, float (&acc)[NB][NR]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 512 + lane * 8;
    float wf[NR][8];
#pragma unroll
    for (int r = 0; r < NR; ++r) unpack8(pre.w[it][r], wf[r]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float xf[8];
      unpack8(*reinterpret_cast<const u32x4_t*>(xs + (size_t)b * K + (c < K ? c : 0)), xf);
      if (c >= K) {
#pragma unroll
        for (int i = 0; i < 8; ++i) xf[i] = 0.f;
      }
#pragma unroll
      for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[b][r] = fmaf(wf[r][i], xf[i], acc[b][r]);
      }
    }
  }
}

template <int NB, int NR, int PRE>
__device__ __forceinline__ void wave_dots_b(const bf16_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NB][NR], WPre<NR, PRE>& pre) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[b][r] = 0.f;
  fma_batch_b<NB, NR, PRE>(pre, xs, 0, K, acc);
  for (int base = PRE * 512; base < K; base += PRE * 512) {
    preload_w<NR, PRE>(wr, base, K, pre);
    __builtin_amdgcn_sched_barrier(0);
    fma_batch_b<NB, NR, PRE>(pre, xs, base, K, acc);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[b][r] = wave_sum(acc[b][r]);
}

// ---------------------------------------------------------------- embedding gather
__global__ __launch_bounds__(256) void decb_embed_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ table,
                                                         bf16_t* __restrict__ x, int ldx, int cols, int n_rows) {
  const svlm_lane& L = lanes[blockIdx.y];
  if (!lane_live(L)) return;
  int id = L.tok_buf[L.state[1]];
  id = min(max(id, 0), n_rows - 1);
  const int c = (blockIdx.x * 256 + threadIdx.x) * 8;
  if (c < cols)
    *reinterpret_cast<u32x4_t*>(x + (size_t)blockIdx.y * ldx + c) = *reinterpret_cast<const u32x4_t*>(table + (size_t)id * cols + c);
}

// ---------------------------------------------------------------- QKV + KV append
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_qkv_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                       const bf16_t* __restrict__ ln_w, float eps, const bf16_t* __restrict__ W, int ldw,
                                                       const bf16_t* __restrict__ bias, bf16_t* __restrict__ q_out, int ldq, int layer,
                                                       int N, int K, int qd, int kd, int D) {
  decb_qkv_body<WBf16, NB, PRE, XC>(lanes, x, ldx, ln_w, eps, W, ldw, /* S: none */ nullptr, bias, q_out, ldq, layer, N, K, qd, kd, D);
}

// ---------------------------------------------------------------- gate/up + SwiGLU
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_gate_up_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ ln_w, float eps, const bf16_t* __restrict__ W, int ldw,
                                                           bf16_t* __restrict__ h, int ldh, int I, int K) {
  decb_gate_up_body<WBf16, NB, PRE, XC>(lanes, x, ldx, ln_w, eps, W, ldw, /* S: none */ nullptr, h, ldh, I, K);
}

// ---------------------------------------------------------------- lm_head + penalty + argmax candidates
#define DECB_LM_ROWS 2            // = LM_ROWS of decode_fused.hip: the candidates are per workgroup of 4 x LM_ROWS vocabulary rows
// (SMP, the Gumbel candidates of svlm_decb_lm_head_sample: decb_lm_head_body, dec_shell.h)
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_lm_head_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ ln_w, float eps, const bf16_t* __restrict__ W, int ldw,
                                                           float* __restrict__ logits, int ldl, const int* __restrict__ suppress,
                                                           float* __restrict__ ws, long long ws_stride, int V, int K) {
  decb_lm_head_body<WBf16, NB, DECB_LM_ROWS, PRE, XC, false>(lanes, nullptr, x, ldx, ln_w, eps, W, ldw, /* S: none */ nullptr, logits, ldl, suppress, ws, ws_stride,
                                                             V, K);
}

template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_lm_head_sample_kernel(const svlm_lane* __restrict__ lanes,
                                                                  const svlm_lane_sample* __restrict__ samples, const bf16_t* __restrict__ x,
                                                                  int ldx, const bf16_t* __restrict__ ln_w, float eps,
                                                                  const bf16_t* __restrict__ W, int ldw, float* __restrict__ logits, int ldl,
                                                                  const int* __restrict__ suppress, float* __restrict__ ws,
                                                                  long long ws_stride, int V, int K) {
  decb_lm_head_body<WBf16, NB, DECB_LM_ROWS, PRE, XC, true>(lanes, samples, x, ldx, ln_w, eps, W, ldw, /* S: none */ nullptr, logits, ldl, suppress, ws, ws_stride,
                                                            V, K);
}

__global__ __launch_bounds__(1024) void decb_argmax_finish_kernel(const svlm_lane* __restrict__ lanes, const float* __restrict__ ws,
                                                                  long long ws_stride, int n_parts, int advance_kv) {
  const svlm_lane& L = lanes[blockIdx.x];
  if (!lane_live(L)) return;
  const float* pv = reinterpret_cast<const float*>(reinterpret_cast<const char*>(ws) + (size_t)blockIdx.x * ws_stride);
  argmax_finish_body(pv, reinterpret_cast<const int*>(pv + n_parts), n_parts, L.seen, L.tok_buf, L.state, advance_kv);
}

// One workgroup per lane, ONE kernel that branches on the lane's mode (workgroup-uniform): a batch is at most 4 workgroups, so the
// 35 KB of static LDS the filtered body brings to every workgroup costs no occupancy, and the lanes' draws run side by side in one
// launch whatever mix of modes the batch holds.
__global__ __launch_bounds__(SF_THREADS) void decb_sample_finish_kernel(const svlm_lane* __restrict__ lanes,
                                                                        const svlm_lane_sample* __restrict__ samples,
                                                                        const float* __restrict__ logits, int ldl,
                                                                        const int* __restrict__ suppress, const float* __restrict__ ws,
                                                                        long long ws_stride, int n_parts, int V, int advance_kv) {
  const svlm_lane& L = lanes[blockIdx.x];
  if (!lane_live(L)) return;
  const svlm_lane_sample& S = samples[blockIdx.x];
  const float* row = logits + (size_t)blockIdx.x * ldl;
  if (S.mode == SVLM_SAMPLE_FILTERED) {
    sample_filtered_body(row, V, L.seen, L.penalty, suppress, L.n_suppress, S.inv_temp, S.top_k, S.top_p, S.rng, L.seen, L.tok_buf, L.state,
                         advance_kv);
  } else if (S.mode == SVLM_SAMPLE_NUCLEUS) {
    sample_nucleus_body(row, V, L.seen, L.penalty, suppress, L.n_suppress, S.inv_temp, S.top_k, S.top_p, S.rng, L.seen, L.tok_buf, L.state,
                        advance_kv);
  } else {
    const float* pv = reinterpret_cast<const float*>(reinterpret_cast<const char*>(ws) + (size_t)blockIdx.x * ws_stride);
    argmax_finish_body(pv, reinterpret_cast<const int*>(pv + n_parts), n_parts, L.seen, L.tok_buf, L.state, advance_kv);
  }
}

// ---------------------------------------------------------------- residual GEMVs (o_proj, down_proj)
// y[b][n] = bf16(bf16(W[n] . x[b]) + residual[b][n]); `y` may be `residual` (in place).  Per (lane, row) the loop of gemv_bf16_kernel.
template <int NB, int ROWS>
__global__ __launch_bounds__(256) void decb_gemv_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                        const bf16_t* __restrict__ W, int ldw, const bf16_t* residual, int ldr, bf16_t* y,
                                                        int ldy, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  if (n0 >= N) return;
  const bf16_t* wr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wr[r] = W + (size_t)min(n0 + r, N - 1) * ldw;
  bool live[NB];
  float acc[NB][ROWS];
  bf16_t epi_raw[NB][ROWS];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    live[b] = lane_live(lanes[b]);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      acc[b][r] = 0.f;
      epi_raw[b][r] = residual[(size_t)b * ldr + min(n0 + r, N - 1)];
    }
  }
  constexpr int PRE = 4;
  for (int base = 0; base < K; base += PRE * 512) {
    u32x4_t xv[PRE][NB], wv[PRE][ROWS];
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 512 + lane * 8;
      const int cc = c < K ? c : 0;
#pragma unroll
      for (int b = 0; b < NB; ++b) xv[it][b] = *reinterpret_cast<const u32x4_t*>(x + (size_t)b * ldx + cc);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) wv[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + cc));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 512 + lane * 8;
      float wf[ROWS][8];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) unpack8(wv[it][r], wf[r]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float xf[8];
        unpack8(xv[it][b], xf);
        if (c >= K) {
#pragma unroll
          for (int i = 0; i < 8; ++i) xf[i] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[b][r] = fmaf(wf[r][i], xf[i], acc[b][r]);
        }
      }
    }
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[b][r] = wave_sum(acc[b][r]);
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (!live[b]) continue;
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int n = n0 + r;
        if (n >= N) break;
        y[(size_t)b * ldy + n] = resid_tail(acc[b][r], epi_raw[b][r]);
      }
    }
  }
}

// Long-K form (down_proj): the 4 waves of a workgroup take a quarter of K each for the same ROWS rows, as gemv_bf16_ksplit_kernel;
// the quarters are summed in the same order.
template <int NB, int ROWS>
__global__ __launch_bounds__(256) void decb_gemv_ksplit_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                               const bf16_t* __restrict__ W, int ldw, const bf16_t* residual, int ldr,
                                                               bf16_t* y, int ldy, int N, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * ROWS;
  const int kq = ((K / 8 + 3) / 4) * 8;
  const int k_lo = wave * kq, k_hi = min(K, k_lo + kq);
  const bf16_t* wr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wr[r] = W + (size_t)min(n0 + r, N - 1) * ldw;
  float acc[NB][ROWS];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[b][r] = 0.f;
  // thread t < NB * ROWS finishes (lane t / ROWS, row t % ROWS); its residual is requested up front
  const int eb = min((int)threadIdx.x / ROWS, NB - 1), er = threadIdx.x % ROWS;
  const bf16_t epi_raw = residual[(size_t)eb * ldr + min(n0 + er, N - 1)];
  constexpr int PRE = 4;
  for (int base = k_lo; base < k_hi; base += PRE * 512) {
    u32x4_t xv[PRE][NB], wv[PRE][ROWS];
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 512 + lane * 8;
      const int cc = c < k_hi ? c : k_lo;
#pragma unroll
      for (int b = 0; b < NB; ++b) xv[it][b] = *reinterpret_cast<const u32x4_t*>(x + (size_t)b * ldx + cc);
#pragma unroll
      for (int r = 0; r < ROWS; ++r) wv[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + cc));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 512 + lane * 8;
      float wf[ROWS][8];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) unpack8(wv[it][r], wf[r]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float xf[8];
        unpack8(xv[it][b], xf);
        if (c >= k_hi) {
#pragma unroll
          for (int i = 0; i < 8; ++i) xf[i] = 0.f;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
#pragma unroll
          for (int i = 0; i < 8; ++i) acc[b][r] = fmaf(wf[r][i], xf[i], acc[b][r]);
        }
      }
    }
  }
  __shared__ float part[4][NB][ROWS];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const float s = wave_sum(acc[b][r]);
      if (lane == 0) part[wave][b][r] = s;
    }
  __syncthreads();
  if (threadIdx.x < NB * ROWS) {
    const int n = n0 + er;
    if (n < N && lane_live(lanes[eb])) {
      y[(size_t)eb * ldy + n] = resid_tail(part[0][eb][er] + part[1][eb][er] + part[2][eb][er] + part[3][eb][er], epi_raw);
    }
  }
}

// ================================================================ launchers
// the NB staged rows share the 64 KB of dynamic LDS a launch gets without opting in
static inline bool decb_ok(int B, int K, int ldx) { return B >= 1 && B <= 4 && K > 0 && K % 8 == 0 && K <= 8192 && B * K * 2 <= 65536 && ldx >= K && ldx % 8 == 0; }

#define DECB_K(KERNEL, NB, K, ...)                                          \
  do {                                                                      \
    if ((K) <= 1536) KERNEL<NB, 3, 1> __VA_ARGS__;                          \
    else if ((K) <= 2048) KERNEL<NB, 4, 1> __VA_ARGS__;                     \
    else if ((K) <= 4096) KERNEL<NB, 4, 2> __VA_ARGS__;                     \
    else KERNEL<NB, 4, 4> __VA_ARGS__;                                      \
  } while (0)
// The two launches whose geometry is one grid row / one workgroup PER LANE and nothing else of B: the entries below keep B <= 4, the
// wide entries (decode_wide.hip) check 1..16 and launch the same kernels through these (declared in dec_lanes.h).
void decb_embed_launch(const void* lanes, int B, const void* table, int n_rows, void* x, int ldx, int cols, void* stream) {
  decb_embed_kernel<<<dim3((cols / 8 + 255) / 256, B), 256, 0, (hipStream_t)stream>>>((const svlm_lane*)lanes, (const bf16_t*)table,
                                                                                      (bf16_t*)x, ldx, cols, n_rows);
}
void decb_argmax_finish_launch(const void* lanes, int B, const void* ws, int V, int advance_kv, void* stream) {
  const int nb = (V + 4 * DECB_LM_ROWS - 1) / (4 * DECB_LM_ROWS);
  decb_argmax_finish_kernel<<<B, 1024, 0, (hipStream_t)stream>>>((const svlm_lane*)lanes, (const float*)ws, svlm_decb_lm_head_ws_stride(V), nb,
                                                                 advance_kv);
}

extern "C" int svlm_decb_embed(const void* lanes, int B, const void* table, int n_rows, void* x, int ldx, int cols, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && B >= 1 && B <= 4 && n_rows > 0 && cols > 0 && cols % 8 == 0 && ldx >= cols && ldx % 8 == 0,
                 "svlm_decb_embed: bad B=%d n_rows=%d cols=%d ldx=%d", B, n_rows, cols, ldx);
  decb_embed_launch(lanes, B, table, n_rows, x, ldx, cols, stream);
  return svlm_check_launch("svlm_decb_embed");
}

extern "C" int svlm_decb_qkv(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W, int ldw,
                             const void* bias, void* q_out, int ldq, int layer, int K, int qd, int kd, int D, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0, "svlm_decb_qkv: bad B=%d K=%d ldx=%d ldw=%d", B, K, ldx, ldw);
  if (!decb_qkv_args_ok("svlm_decb_qkv", qd, kd, D, bias, ldq, layer)) return SVLM_EINVAL;
  const int N = qd + 2 * kd;
  DECB_SWITCH_NB(B, DECB_K(decb_qkv_kernel, NB, K, <<<(N + 3) / 4, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, (const bf16_t*)bias, (bf16_t*)q_out, ldq,
      layer, N, K, qd, kd, D)));
  return svlm_check_launch("svlm_decb_qkv");
}

extern "C" int svlm_decb_gate_up(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W, int ldw,
                                 void* h, int ldh, int I, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0 && I > 0 && ldh >= I,
                 "svlm_decb_gate_up: bad B=%d I=%d K=%d ldx=%d ldw=%d ldh=%d", B, I, K, ldx, ldw, ldh);
  DECB_SWITCH_NB(B, DECB_K(decb_gate_up_kernel, NB, K, <<<(I + 3) / 4, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, (bf16_t*)h, ldh, I, K)));
  return svlm_check_launch("svlm_decb_gate_up");
}

extern "C" int svlm_decb_gemv(const void* lanes, int B, const void* x, int ldx, const void* W, int ldw, const void* residual, int ldr,
                              void* y, int ldy, int N, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && B >= 1 && B <= 4 && N > 0 && K > 0 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K && ldx >= K && ldx % 8 == 0,
                 "svlm_decb_gemv: bad shape B=%d N=%d K=%d ldw=%d ldx=%d", B, N, K, ldw, ldx);
  SVLM_CHECK_ARG(residual != nullptr && y != nullptr && ldr >= N && ldy >= N, "svlm_decb_gemv: residual and y are required (ldr=%d ldy=%d)", ldr, ldy);
  hipStream_t s = (hipStream_t)stream;
  if (N <= 8192 && K >= 4096) {        // the shapes svlm_gemv_bf16 splits over K
    DECB_SWITCH_NB(B, decb_gemv_ksplit_kernel<NB, 2><<<(N + 1) / 2, 256, 0, s>>>((const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)W, ldw,
                                                                        (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, N, K));
    return svlm_check_launch("svlm_decb_gemv(ksplit)");
  }
  if (N >= 4096 || (long long)N * K >= (8LL << 20)) {
    DECB_SWITCH_NB(B, decb_gemv_kernel<NB, 2><<<(N + 7) / 8, 256, 0, s>>>((const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)W, ldw,
                                                                 (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, N, K));
  } else {
    DECB_SWITCH_NB(B, decb_gemv_kernel<NB, 1><<<(N + 3) / 4, 256, 0, s>>>((const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)W, ldw,
                                                                 (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, N, K));
  }
  return svlm_check_launch("svlm_decb_gemv");
}

extern "C" long long svlm_decb_lm_head_ws_stride(int V) {
  if (V <= 0) return SVLM_EINVAL;
  const long long nb = (V + 4 * DECB_LM_ROWS - 1) / (4 * DECB_LM_ROWS);
  return (nb * 8 + 15) / 16 * 16;
}

extern "C" int svlm_decb_lm_head(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W, int ldw,
                                 float* logits, int ldl, const int* suppress, void* ws, int V, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0 && V > 0 && ldl >= V,
                 "svlm_decb_lm_head: bad B=%d V=%d K=%d ldx=%d ldw=%d ldl=%d", B, V, K, ldx, ldw, ldl);
  SVLM_CHECK_ARG(ws != nullptr && logits != nullptr, "svlm_decb_lm_head: null logits / workspace");
  const int nb = (V + 4 * DECB_LM_ROWS - 1) / (4 * DECB_LM_ROWS);
  DECB_SWITCH_NB(B, DECB_K(decb_lm_head_kernel, NB, K, <<<nb, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, logits, ldl, suppress, (float*)ws,
      svlm_decb_lm_head_ws_stride(V), V, K)));
  return svlm_check_launch("svlm_decb_lm_head");
}

extern "C" int svlm_decb_argmax_finish(const void* lanes, int B, const void* ws, int V, int advance_kv, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && B >= 1 && B <= 4 && V > 0 && ws != nullptr, "svlm_decb_argmax_finish: bad args");
  decb_argmax_finish_launch(lanes, B, ws, V, advance_kv, stream);
  return svlm_check_launch("svlm_decb_argmax_finish");
}

extern "C" int svlm_decb_lm_head_sample(const void* lanes, const void* samples, int B, const void* x, int ldx, const void* ln_w, float eps,
                                        const void* W, int ldw, float* logits, int ldl, const int* suppress, void* ws, int V, int K,
                                        void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && samples != nullptr && decb_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0 && V > 0 && ldl >= V,
                 "svlm_decb_lm_head_sample: bad B=%d V=%d K=%d ldx=%d ldw=%d ldl=%d or no lane / sample table", B, V, K, ldx, ldw, ldl);
  SVLM_CHECK_ARG(ws != nullptr && logits != nullptr, "svlm_decb_lm_head_sample: null logits / workspace");
  const int nb = (V + 4 * DECB_LM_ROWS - 1) / (4 * DECB_LM_ROWS);
  DECB_SWITCH_NB(B, DECB_K(decb_lm_head_sample_kernel, NB, K, <<<nb, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const svlm_lane_sample*)samples, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, logits,
      ldl, suppress, (float*)ws, svlm_decb_lm_head_ws_stride(V), V, K)));
  return svlm_check_launch("svlm_decb_lm_head_sample");
}

extern "C" int svlm_decb_sample_finish(const void* lanes, const void* samples, int B, const float* logits, int ldl, const int* suppress,
                                       const void* ws, int V, int advance_kv, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && samples != nullptr && B >= 1 && B <= 4 && V > 0 && ws != nullptr && logits != nullptr && ldl >= V,
                 "svlm_decb_sample_finish: bad B=%d V=%d ldl=%d or a null table / logits / workspace", B, V, ldl);
  // the row scan takes 16-B loads when V is a multiple of 4: every lane's row must then start on a 16-B boundary
  SVLM_CHECK_ARG(V % 4 != 0 || (ldl % 4 == 0 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0),
                 "svlm_decb_sample_finish: logits rows of V=%d need a 16-B aligned base and ldl=%d a multiple of 4", V, ldl);
  const int nb = (V + 4 * DECB_LM_ROWS - 1) / (4 * DECB_LM_ROWS);
  decb_sample_finish_kernel<<<B, SF_THREADS, 0, (hipStream_t)stream>>>((const svlm_lane*)lanes, (const svlm_lane_sample*)samples, logits, ldl,
                                                                       suppress, (const float*)ws, svlm_decb_lm_head_ws_stride(V), nb, V,
                                                                       advance_kv);
  return svlm_check_launch("svlm_decb_sample_finish");
}
