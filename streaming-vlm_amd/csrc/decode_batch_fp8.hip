// Lane-batched decode-step kernels on OCP e4m3 weights with one power-of-two scale per output row: stream groups (stream_group.py)
// on an `llm_fp8` engine.  The fused kernels are the lane-batched shells of dec_shell.h over the policy WFp8 (dec_fp8.h) around this
// file's K loop (cvt16, fma_batch8_b, wave_dots8_b), with the epilogue pieces of the single-row kernels (dec_epi.h); the lm_head and the
// residual GEMV keep bodies of their own (on the shared ones some instantiations took up to 26 more VGPRs).  Entry, its single-row counterpart:
//
//   svlm_decb_qkv_fp8      svlm_dec_qkv_fp8       RMSNorm + QKV + bias + KV append to each lane's own pool slot / linear planes
//   svlm_decb_gate_up_fp8  svlm_dec_gate_up_fp8   RMSNorm + gate/up + SwiGLU
//   svlm_decb_gemv_fp8     svlm_gemv_fp8          o_proj / down_proj + residual, every dispatch branch of the single-row entry
//   svlm_decb_lm_head_fp8  svlm_dec_lm_head_fp8   greedy: penalty, suppression, argmax candidates per lane (svlm_decb_argmax_finish and
//                                                 svlm_decb_lm_head_ws_stride of decode_batch.hip serve unchanged)
//   svlm_decb_lm_head_sample_fp8  svlm_dec_lm_head_sample_fp8  the same with Gumbel noise in the candidates of the lanes whose sampling
//                                                 record says so (completed by svlm_decb_sample_finish of decode_batch.hip)
//
// A wave loads its weight rows once (16-B non-temporal loads straight to VGPRs, every load of a batch issued before its first FMA),
// converts each 16-code vector to fp32 ONCE and multiplies the converted values with the NB activation rows of the group: the batch
// amortises the e4m3 -> fp32 conversion as well as the weight bytes.
//
// ARITHMETIC ORDER IS KEPT PER LANE: for one (lane, output row) the FMA sequence over K (dot16's element order, 1024-element K-steps
// with 16 consecutive elements per thread), wave_sum, the K-split bounds and the partial sum order, the scale applied once in the
// epilogue and every bf16 rounding point are those of the single-row fp8 kernel (shared through dec_fp8.h / dec_xrow.h), so every
// output is bitwise the single-row kernel's.  The conversion is exact, so converting once or once per lane gives the same factors.
// How many rows a wave takes, and PRE, do not enter a row's arithmetic; only the lm_head keeps the single-row kernel's 8 vocabulary
// rows per workgroup, because the candidates are per workgroup.
//
// A lane that is not live (state[1] + 1 >= limit) is skipped by every kernel: no KV row, no token, no output row written.
#include "common.h"
#include "dec_xrow.h"
#include "dec_fp8.h"
#include "dec_lanes.h"
#include "dec_launch.h"           // host side: lane-count switch, qkv argument checks
#include "dec_shell.h"            // the kernel shells over WFp8 (dec_fp8.h); epilogue pieces: dec_epi.h

// the 16 codes of one 16-B weight vector as fp32, in element order (the factors dot16 feeds its FMAs with)
__device__ __forceinline__ void cvt16(const u32x4_t& w, float (&wf)[16]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    wf[4 * i] = lo[0];
    wf[4 * i + 1] = lo[1];
    wf[4 * i + 2] = hi[0];
    wf[4 * i + 3] = hi[1];
  }
}
// dot16 on converted codes: the same 16 FMAs in the same order
__device__ __forceinline__ float dot16f(const float (&wf)[16], const float (&xf)[16], float acc) {
#pragma unroll
  for (int i = 0; i < 16; ++i) acc = fmaf(wf[i], xf[i], acc);
  return acc;
}

// acc[b][r] += q[row r] . xs[b] over the PRE K-steps held in `pre`; per (b, r) the FMA sequence of fma_batch8 (decode_fp8.hip)
template <int NB, int NR, int PRE>
__device__ __forceinline__ void fma_batch8_b(const W8Pre<NR, PRE>& pre, const bf16_t* xs, int base, int K, float (&acc)[NB][NR]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 1024 + lane * 16;
    float wf[NR][16];
#pragma unroll
    for (int r = 0; r < NR; ++r) cvt16(pre.w[it][r], wf[r]);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      float xf[16];
      x16(xs + (size_t)b * K, c, K, xf);
#pragma unroll
      for (int r = 0; r < NR; ++r) acc[b][r] = dot16f(wf[r], xf, acc[b][r]);
    }
  }
}

template <int NB, int NR, int PRE>
__device__ __forceinline__ void wave_dots8_b(const fp8_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NB][NR], W8Pre<NR, PRE>& pre) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[b][r] = 0.f;
  fma_batch8_b<NB, NR, PRE>(pre, xs, 0, K, acc);
  for (int base = PRE * 1024; base < K; base += PRE * 1024) {
    preload_w8<NR, PRE>(wr, base, K, pre);
    __builtin_amdgcn_sched_barrier(0);                       // every load of the batch is issued before its first FMA
    fma_batch8_b<NB, NR, PRE>(pre, xs, base, K, acc);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[b][r] = wave_sum(acc[b][r]);
}

// ---------------------------------------------------------------- QKV + KV append
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_qkv_fp8_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ ln_w, float eps, const fp8_t* __restrict__ W, int ldw,
                                                           const float* __restrict__ w_scale, const bf16_t* __restrict__ bias,
                                                           bf16_t* __restrict__ q_out, int ldq, int layer, int N, int K, int qd, int kd,
                                                           int D) {
  decb_qkv_body<WFp8, NB, PRE, XC>(lanes, x, ldx, ln_w, eps, W, ldw, w_scale, bias, q_out, ldq, layer, N, K, qd, kd, D);
}

// ---------------------------------------------------------------- gate/up + SwiGLU
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_gate_up_fp8_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                               const bf16_t* __restrict__ ln_w, float eps, const fp8_t* __restrict__ W,
                                                               int ldw, const float* __restrict__ w_scale, bf16_t* __restrict__ h, int ldh,
                                                               int I, int K) {
  decb_gate_up_body<WFp8, NB, PRE, XC>(lanes, x, ldx, ln_w, eps, W, ldw, w_scale, h, ldh, I, K);
}

// ---------------------------------------------------------------- lm_head + penalty + argmax candidates
#define DECB_LM8_ROWS 2           // = LM8_ROWS of decode_fp8.hip = DECB_LM_ROWS of decode_batch.hip: one candidate per 8 vocabulary rows
// The e4m3 head keeps a shell of its own, with the epilogue pieces of dec_epi.h: on decb_lm_head_body (dec_shell.h) over WFp8 its
// K <= 1024 forms took more registers (<2, 1, 1> 86 -> 91 VGPRs, <3, 1, 1> 87 -> 110) and the three-lane one ran 9 % slower.
// SMP: a live lane in Gumbel mode gets score * inv_temp + noise as its candidate score (cand_score).
template <int NB, int PRE, int XC, bool SMP>
__device__ __forceinline__ void decb_lm_head_fp8_body(const svlm_lane* __restrict__ lanes, const svlm_lane_sample* __restrict__ samples,
                                                      const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ ln_w, float eps,
                                                      const fp8_t* __restrict__ W, int ldw, const float* __restrict__ w_scale,
                                                      float* __restrict__ logits, int ldl, const int* __restrict__ suppress,
                                                      float* __restrict__ ws, long long ws_stride, int V, int K) {
  constexpr int ROWS = DECB_LM8_ROWS;
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  const fp8_t* wr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wr[r] = W + (size_t)min(n0 + r, V - 1) * ldw;
  XRow<XC> xr[NB];
  bool live[NB];
  load_rows<NB, XC>(lanes, x, ldx, ln_w, K, xr, live);
  __builtin_amdgcn_sched_barrier(0);
  W8Pre<ROWS, PRE> pre;
  preload_w8<ROWS, PRE>(wr, 0, K, pre);
  float spre[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) spre[r] = w_scale[min(n0 + r, V - 1)];
  __builtin_amdgcn_sched_barrier(0);
  stage_rows<NB, XC>(xr, live, eps, K, xs);
  float best[NB];
  int bi[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) { best[b] = -INFINITY; bi[b] = 0x7fffffff; }
  if (n0 < V) {
    float acc[NB][ROWS];
    wave_dots8_b<NB, ROWS, PRE>(wr, xs, K, acc, pre);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (!live[b]) continue;
      const svlm_lane& L = lanes[b];
      const unsigned* rng = nullptr;
      float inv_temp = 1.0f;
      if constexpr (SMP) {
        if (samples[b].mode == SVLM_SAMPLE_GUMBEL) { rng = samples[b].rng; inv_temp = samples[b].inv_temp; }
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) {
        const int n = n0 + r;
        if (n >= V) break;
        float v = rbf(acc[b][r] * spre[r]);
        if (lane == 0) logits[(size_t)b * ldl + n] = v;
        v = cand_score(v, n, L.seen, L.penalty, suppress, L.n_suppress, rng, inv_temp, L.state);
        cand_take(best[b], bi[b], v, n);
      }
    }
  }
  float bb;
  int ii;
  if (cand_reduce<NB>(best, bi, bb, ii) && lane_live(lanes[threadIdx.x])) {
    float* pv = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + (size_t)threadIdx.x * ws_stride);
    int* pi = reinterpret_cast<int*>(pv + gridDim.x);
    pv[blockIdx.x] = bb;
    pi[blockIdx.x] = ii;
  }
}

template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_lm_head_fp8_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                               const bf16_t* __restrict__ ln_w, float eps, const fp8_t* __restrict__ W,
                                                               int ldw, const float* __restrict__ w_scale, float* __restrict__ logits,
                                                               int ldl, const int* __restrict__ suppress, float* __restrict__ ws,
                                                               long long ws_stride, int V, int K) {
  decb_lm_head_fp8_body<NB, PRE, XC, false>(lanes, nullptr, x, ldx, ln_w, eps, W, ldw, w_scale, logits, ldl, suppress, ws, ws_stride, V, K);
}

template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_lm_head_sample_fp8_kernel(const svlm_lane* __restrict__ lanes,
                                                                      const svlm_lane_sample* __restrict__ samples,
                                                                      const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ ln_w,
                                                                      float eps, const fp8_t* __restrict__ W, int ldw,
                                                                      const float* __restrict__ w_scale, float* __restrict__ logits, int ldl,
                                                                      const int* __restrict__ suppress, float* __restrict__ ws,
                                                                      long long ws_stride, int V, int K) {
  decb_lm_head_fp8_body<NB, PRE, XC, true>(lanes, samples, x, ldx, ln_w, eps, W, ldw, w_scale, logits, ldl, suppress, ws, ws_stride, V, K);
}

// ---------------------------------------------------------------- residual GEMVs (o_proj, down_proj)
// y[b][n] = bf16(bf16(q[n] . x[b] * s[n]) + residual[b][n]); `y` may be `residual` (in place).  Per (lane, row) the loop of
// gemv_fp8_kernel: the 4 waves of a workgroup form 4 / KW groups of ROWS rows, the KW waves of a group take one 1/KW share of K each
// and the shares are summed partial[w] + partial[w + 1] + ...  The NB x rows come from global memory (a down_proj row of 4 lanes does
// not fit a workgroup's LDS share, and the rows are L2-resident).
template <int NB, int ROWS, int KW, int PRE>
__global__ __launch_bounds__(256) void decb_gemv_fp8_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                            const fp8_t* __restrict__ W, int ldw, const float* __restrict__ w_scale,
                                                            const bf16_t* residual, int ldr, bf16_t* y, int ldy, int N, int K) {
  static_assert(KW == 1 || KW == 4, "one group per wave, or one group per workgroup");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave / KW, part = wave % KW;
  const int n0 = (blockIdx.x * (4 / KW) + grp) * ROWS;
  const int kq = ((K / 16 + KW - 1) / KW) * 16;        // elements per wave (multiple of 16)
  const int k_lo = part * kq, k_hi = min(K, k_lo + kq);
  const fp8_t* wr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) wr[r] = W + (size_t)min(n0 + r, N - 1) * ldw;
  float acc[NB][ROWS];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[b][r] = 0.f;
  // thread t < NB * ROWS of a group's first wave finishes (lane t / ROWS, row t % ROWS); its residual and scale are requested up
  // front, their latency hides under the weight stream
  const int eb = min(lane / ROWS, NB - 1), er = lane % ROWS;
  const bf16_t epi_raw = residual[(size_t)eb * ldr + min(n0 + er, N - 1)];
  const float spre = w_scale[min(n0 + er, N - 1)];
  for (int base = k_lo; base < k_hi; base += PRE * 1024) {
    u32x4_t xa[PRE][NB], xb[PRE][NB], wv[PRE][ROWS];
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 1024 + lane * 16;
      const int cc = c < k_hi ? c : k_lo;
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        xa[it][b] = *reinterpret_cast<const u32x4_t*>(x + (size_t)b * ldx + cc);
        xb[it][b] = *reinterpret_cast<const u32x4_t*>(x + (size_t)b * ldx + cc + 8);
      }
#pragma unroll
      for (int r = 0; r < ROWS; ++r) wv[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + cc));
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const bool in = base + it * 1024 + lane * 16 < k_hi;
      float wf[ROWS][16];
#pragma unroll
      for (int r = 0; r < ROWS; ++r) cvt16(wv[it][r], wf[r]);
#pragma unroll
      for (int b = 0; b < NB; ++b) {
        float lo[8], hi[8], xf[16];
        unpack8(xa[it][b], lo);
        unpack8(xb[it][b], hi);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          xf[i] = in ? lo[i] : 0.f;
          xf[8 + i] = in ? hi[i] : 0.f;
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r) acc[b][r] = dot16f(wf[r], xf, acc[b][r]);
      }
    }
  }
  __shared__ float partial[4][NB][ROWS];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const float s = wave_sum(acc[b][r]);
      if (lane == 0) partial[wave][b][r] = s;
    }
  if (KW > 1) __syncthreads();
  else lds_barrier();                                  // (a wave reads what its own lane 0 wrote)
  if (part != 0 || lane >= NB * ROWS) return;
  const int n = n0 + er;
  if (n >= N || !lane_live(lanes[eb])) return;
  float s = partial[wave][eb][er];
#pragma unroll
  for (int p = 1; p < KW; ++p) s += partial[wave + p][eb][er];
  y[(size_t)eb * ldy + n] = resid_tail(s * spre, epi_raw);
}

// ================================================================ launchers
// the NB staged rows fit the 64 KB of LDS a workgroup gets without opting in, less the kernels' own static reduction arrays (at most
// 144 B, the lm_head's candidates): B * K * 2 may reach 65536 - 256
static inline bool decb8_ok(int B, int K, int ldx, int ldw) {
  return B >= 1 && B <= 4 && K > 0 && K % 16 == 0 && K <= 8192 && B * K * 2 <= 65536 - 256 && ldx >= K && ldx % 8 == 0 && ldw >= K && ldw % 16 == 0;
}

// (PRE, XC) by row length, as DEC8_DISPATCH of decode_fp8.hip
#define DECB8_K(KERNEL, NB, K, ...)                                         \
  do {                                                                      \
    if ((K) <= 1024) KERNEL<NB, 1, 1> __VA_ARGS__;                          \
    else if ((K) <= 2048) KERNEL<NB, 2, 1> __VA_ARGS__;                     \
    else if ((K) <= 4096) KERNEL<NB, 4, 2> __VA_ARGS__;                     \
    else KERNEL<NB, 4, 4> __VA_ARGS__;                                      \
  } while (0)
extern "C" int svlm_decb_qkv_fp8(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W8, int ldw,
                                 const float* w_scale, const void* bias, void* q_out, int ldq, int layer, int K, int qd, int kd, int D,
                                 void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb8_ok(B, K, ldx, ldw) && w_scale != nullptr,
                 "svlm_decb_qkv_fp8: bad B=%d K=%d ldx=%d ldw=%d (B 1..4, K and ldw multiples of 16, B*K*2 <= 64 KB - 256) or no scales", B, K, ldx, ldw);
  if (!decb_qkv_args_ok("svlm_decb_qkv_fp8", qd, kd, D, bias, ldq, layer)) return SVLM_EINVAL;
  const int N = qd + 2 * kd;
  DECB_SWITCH_NB(B, DECB8_K(decb_qkv_fp8_kernel, NB, K, <<<(N + 3) / 4, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale, (const bf16_t*)bias,
      (bf16_t*)q_out, ldq, layer, N, K, qd, kd, D)));
  return svlm_check_launch("svlm_decb_qkv_fp8");
}

extern "C" int svlm_decb_gate_up_fp8(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W8, int ldw,
                                     const float* w_scale, void* h, int ldh, int I, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb8_ok(B, K, ldx, ldw) && w_scale != nullptr && I > 0 && ldh >= I,
                 "svlm_decb_gate_up_fp8: bad B=%d I=%d K=%d ldx=%d ldw=%d ldh=%d or no scales", B, I, K, ldx, ldw, ldh);
  DECB_SWITCH_NB(B, DECB8_K(decb_gate_up_fp8_kernel, NB, K, <<<(I + 3) / 4, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale, (bf16_t*)h, ldh, I, K)));
  return svlm_check_launch("svlm_decb_gate_up_fp8");
}

extern "C" int svlm_decb_gemv_fp8(const void* lanes, int B, const void* x, int ldx, const void* W8, int ldw, const float* w_scale,
                                  const void* residual, int ldr, void* y, int ldy, int N, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && B >= 1 && B <= 4 && N > 0 && K > 0 && K % 16 == 0 && ldw % 16 == 0 && ldw >= K && ldx >= K &&
                     ldx % 8 == 0 && w_scale != nullptr,
                 "svlm_decb_gemv_fp8: bad shape B=%d N=%d K=%d ldw=%d ldx=%d (multiples of 16) or no scales", B, N, K, ldw, ldx);
  SVLM_CHECK_ARG(residual != nullptr && y != nullptr && ldr >= N && ldy >= N, "svlm_decb_gemv_fp8: residual and y are required (ldr=%d ldy=%d)",
                 ldr, ldy);
  hipStream_t s = (hipStream_t)stream;
#define DECB8_GEMV_ARGS (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const fp8_t*)W8, ldw, w_scale, (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, N, K
  // the dispatch of svlm_gemv_fp8, branch for branch (ROWS, KW and the grid; PRE does not enter a row's arithmetic)
  if (N <= 8192 && K >= 4096) {
    DECB_SWITCH_NB(B, decb_gemv_fp8_kernel<NB, 2, 4, 3><<<(N + 1) / 2, 256, 0, s>>>(DECB8_GEMV_ARGS));
  } else if (N >= 16384) {
    DECB_SWITCH_NB(B, decb_gemv_fp8_kernel<NB, 4, 1, 2><<<(N + 15) / 16, 256, 0, s>>>(DECB8_GEMV_ARGS));
  } else if (N >= 4096 || (long long)N * K >= (8LL << 20)) {
    DECB_SWITCH_NB(B, decb_gemv_fp8_kernel<NB, 2, 1, 2><<<(N + 7) / 8, 256, 0, s>>>(DECB8_GEMV_ARGS));
  } else {   // 3 and 4 lanes: two K-steps in flight instead of four, whose x vectors (PRE x NB x 32 B per thread) cost the occupancy
    DECB_SWITCH_NB(B, decb_gemv_fp8_kernel<NB, 1, 1, (NB <= 2 ? 4 : 2)><<<(N + 3) / 4, 256, 0, s>>>(DECB8_GEMV_ARGS));
  }
#undef DECB8_GEMV_ARGS
  return svlm_check_launch("svlm_decb_gemv_fp8");
}

extern "C" long long svlm_decb_lm_head_ws_stride(int V);

extern "C" int svlm_decb_lm_head_fp8(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W8, int ldw,
                                     const float* w_scale, float* logits, int ldl, const int* suppress, void* ws, int V, int K,
                                     void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb8_ok(B, K, ldx, ldw) && w_scale != nullptr && V > 0 && ldl >= V,
                 "svlm_decb_lm_head_fp8: bad B=%d V=%d K=%d ldx=%d ldw=%d ldl=%d or no scales", B, V, K, ldx, ldw, ldl);
  SVLM_CHECK_ARG(ws != nullptr && logits != nullptr, "svlm_decb_lm_head_fp8: null logits / workspace");
  const int nb = (V + 4 * DECB_LM8_ROWS - 1) / (4 * DECB_LM8_ROWS);
  DECB_SWITCH_NB(B, DECB8_K(decb_lm_head_fp8_kernel, NB, K, <<<nb, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale, logits, ldl, suppress,
      (float*)ws, svlm_decb_lm_head_ws_stride(V), V, K)));
  return svlm_check_launch("svlm_decb_lm_head_fp8");
}

extern "C" int svlm_decb_lm_head_sample_fp8(const void* lanes, const void* samples, int B, const void* x, int ldx, const void* ln_w, float eps,
                                            const void* W8, int ldw, const float* w_scale, float* logits, int ldl, const int* suppress,
                                            void* ws, int V, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && samples != nullptr && decb8_ok(B, K, ldx, ldw) && w_scale != nullptr && V > 0 && ldl >= V,
                 "svlm_decb_lm_head_sample_fp8: bad B=%d V=%d K=%d ldx=%d ldw=%d ldl=%d or no lane / sample table / scales", B, V, K, ldx, ldw, ldl);
  SVLM_CHECK_ARG(ws != nullptr && logits != nullptr, "svlm_decb_lm_head_sample_fp8: null logits / workspace");
  const int nb = (V + 4 * DECB_LM8_ROWS - 1) / (4 * DECB_LM8_ROWS);
  DECB_SWITCH_NB(B, DECB8_K(decb_lm_head_sample_fp8_kernel, NB, K, <<<nb, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const svlm_lane_sample*)samples, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const fp8_t*)W8, ldw, w_scale,
      logits, ldl, suppress, (float*)ws, svlm_decb_lm_head_ws_stride(V), V, K)));
  return svlm_check_launch("svlm_decb_lm_head_sample_fp8");
}
