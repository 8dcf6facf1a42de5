// Lane-batched decode-step kernels on OCP MXFP4 weights (e2m1 codes, two per byte, one e8m0 scale per block of 32 K elements): stream
// groups (stream_group.py) on an `llm_fp4` engine.  The fused kernels are the lane-batched shells of dec_shell.h over the policy WFp4
// (dec_fp4.h) around this file's K loop (cvt16_fp4, fma_batch4_b, wave_dots4_b), with the epilogue pieces of the single-row kernels
// (dec_epi.h); the residual GEMV is this file's own, as in decode_batch_fp8.hip.  Entry, its single-row counterpart:
//
//   svlm_decb_qkv_fp4      svlm_dec_qkv_fp4       RMSNorm + QKV + bias + KV append to each lane's own pool slot / linear planes
//   svlm_decb_gate_up_fp4  svlm_dec_gate_up_fp4   RMSNorm + gate/up + SwiGLU
//   svlm_decb_gemv_fp4     svlm_gemv_fp4          o_proj / down_proj + residual, every dispatch branch of the single-row entry
//
// (The lm_head of an fp4 engine is e4m3: svlm_decb_lm_head[_sample]_fp8 of decode_batch_fp8.hip and the embed / finish entries of
// decode_batch.hip serve unchanged.)
//
// A wave loads its weight rows once (16-B non-temporal loads straight to VGPRs plus one scale byte per load, every load of a batch
// issued before its first FMA), converts each 16-code half block to fp32 ONCE -- eight v_cvt_scalef32_pk_f32_fp4, the block scale
// applied inside the conversion -- and multiplies the converted values with the NB activation rows of the group.
//
// ARITHMETIC ORDER IS KEPT PER LANE: for one (lane, output row) the FMA sequence over K (dot16_fp4's element order, low nibble first;
// 2048-element K-steps with 32 consecutive elements per thread, two half blocks of 16), the masking past K, wave_sum, the GEMV's
// K-split bounds and the partial sum order, and every epilogue expression and bf16 rounding point are those of the single-row fp4
// kernel, so every output is bitwise the single-row kernel's.  The conversion is exact (a power-of-two scale on a code of 2 significant
// bits), so converting once or once per lane gives the same factors.  How many rows a wave takes, PRE, and how the x rows are staged
// do not enter a row's arithmetic.
//
// A lane that is not live (state[1] + 1 >= limit) is skipped by every kernel: no KV row, no output row written.
#include "common.h"
#include "dec_xrow.h"
#include "dec_fp4.h"
#include "dec_lanes.h"
#include "dec_launch.h"           // host side: lane-count switch, qkv argument checks
#include "dec_shell.h"            // the kernel shells over WFp4 (dec_fp4.h); epilogue pieces: dec_epi.h

// the 16 codes of one half block (w0 | w1: 8 bytes) times the block scale, as fp32 in element order: the factors dot16_fp4 feeds its
// FMAs with
__device__ __forceinline__ void cvt16_fp4(unsigned w0, unsigned w1, float s, float (&wf)[16]) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned w = h ? w1 : w0;
    const f32x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 0);
    const f32x2_t b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 1);
    const f32x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 2);
    const f32x2_t d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 3);
    wf[8 * h] = a[0];
    wf[8 * h + 1] = a[1];
    wf[8 * h + 2] = b[0];
    wf[8 * h + 3] = b[1];
    wf[8 * h + 4] = c[0];
    wf[8 * h + 5] = c[1];
    wf[8 * h + 6] = d[0];
    wf[8 * h + 7] = d[1];
  }
}
// dot16_fp4 on converted codes: the same 16 FMAs in the same order
__device__ __forceinline__ float dot16f4(const float (&wf)[16], const float (&xf)[16], float acc) {
#pragma unroll
  for (int i = 0; i < 16; ++i) acc = fmaf(wf[i], xf[i], acc);
  return acc;
}

// acc[b][r] += W'[row r] . xs[b] over the PRE K-steps held in `pre`; per (b, r) the FMA sequence of fma_batch4 (decode_fp4.hip)
template <int NB, int NR, int PRE>
__device__ __forceinline__ void fma_batch4_b(const W4Pre<NR, PRE>& pre, const bf16_t* xs, int base, int K, float (&acc)[NB][NR]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 2048 + lane * 32;
    float s[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) s[r] = e8m0_f32(pre.s[it][r]);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if constexpr (NB == 1) {
        // one lane: nothing to amortise, so the single-row kernel's own form (conversion beside its FMAs: no converted half block
        // held in registers; gate/up takes 66 / 73 VGPRs this way against 105 / 100)
        float xf[16];
        x16(xs, c + 16 * h, K, xf);
#pragma unroll
        for (int r = 0; r < NR; ++r) acc[0][r] = dot16_fp4(pre.w[it][r][2 * h], pre.w[it][r][2 * h + 1], s[r], xf, acc[0][r]);
      } else {
        float wf[NR][16];
#pragma unroll
        for (int r = 0; r < NR; ++r) cvt16_fp4(pre.w[it][r][2 * h], pre.w[it][r][2 * h + 1], s[r], wf[r]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          float xf[16];
          x16(xs + (size_t)b * K, c + 16 * h, K, xf);        // K % 32 == 0: both halves of a block are inside K or neither is
#pragma unroll
          for (int r = 0; r < NR; ++r) acc[b][r] = dot16f4(wf[r], xf, acc[b][r]);
        }
      }
    }
  }
}

template <int NB, int NR, int PRE>
__device__ __forceinline__ void wave_dots4_b(const fp4x2_t* const (&wr)[NR], const e8m0_t* const (&sr)[NR], const bf16_t* xs, int K,
                                             float (&acc)[NB][NR], W4Pre<NR, PRE>& pre) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[b][r] = 0.f;
  fma_batch4_b<NB, NR, PRE>(pre, xs, 0, K, acc);
  for (int base = PRE * 2048; base < K; base += PRE * 2048) {
    preload_w4<NR, PRE>(wr, sr, base, K, pre);
    __builtin_amdgcn_sched_barrier(0);                       // every load of the batch is issued before its first FMA
    fma_batch4_b<NB, NR, PRE>(pre, xs, base, K, acc);
  }
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < NR; ++r) acc[b][r] = wave_sum(acc[b][r]);
}

// ---------------------------------------------------------------- QKV + KV append
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_qkv_fp4_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ ln_w, float eps, const fp4x2_t* __restrict__ W, int ldw,
                                                           const e8m0_t* __restrict__ S, const bf16_t* __restrict__ bias,
                                                           bf16_t* __restrict__ q_out, int ldq, int layer, int N, int K, int qd, int kd,
                                                           int D) {
  decb_qkv_body<WFp4, NB, PRE, XC>(lanes, x, ldx, ln_w, eps, W, ldw, S, bias, q_out, ldq, layer, N, K, qd, kd, D);
}

// ---------------------------------------------------------------- gate/up + SwiGLU
template <int NB, int PRE, int XC>
__global__ __launch_bounds__(256) void decb_gate_up_fp4_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                               const bf16_t* __restrict__ ln_w, float eps, const fp4x2_t* __restrict__ W,
                                                               int ldw, const e8m0_t* __restrict__ S, bf16_t* __restrict__ h, int ldh, int I,
                                                               int K) {
  decb_gate_up_body<WFp4, NB, PRE, XC>(lanes, x, ldx, ln_w, eps, W, ldw, S, h, ldh, I, K);
}

// ---------------------------------------------------------------- residual GEMVs (o_proj, down_proj)
// y[b][n] = bf16(bf16(W'[n] . x[b]) + residual[b][n]); `y` may be `residual` (in place).  Per (lane, row) the loop of gemv_fp4_kernel:
// the 4 waves of a workgroup form 4 / KW groups of ROWS rows, the KW waves of a group take one 1/KW share of K each (whole blocks) and
// the shares are summed partial[w] + partial[w + 1] + ...  The NB x rows come from global memory (a down_proj row of 4 lanes does not
// fit a workgroup's LDS share, and the rows are L2-resident).
template <int NB, int ROWS, int KW, int PRE>
__global__ __launch_bounds__(256) void decb_gemv_fp4_kernel(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                            const fp4x2_t* __restrict__ W, int ldw, const e8m0_t* __restrict__ S,
                                                            const bf16_t* residual, int ldr, bf16_t* y, int ldy, int N, int K) {
  static_assert(KW == 1 || KW == 4, "one group per wave, or one group per workgroup");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int grp = wave / KW, part = wave % KW;
  const int n0 = (blockIdx.x * (4 / KW) + grp) * ROWS;
  const int kq = ((K / 32 + KW - 1) / KW) * 32;        // elements per wave (whole blocks)
  const int k_lo = part * kq, k_hi = min(K, k_lo + kq);
  const fp4x2_t* wr[ROWS];
  const e8m0_t* sr[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = min(n0 + r, N - 1);
    wr[r] = W + (size_t)n * ldw;
    sr[r] = S + (size_t)n * (K >> 5);
  }
  float acc[NB][ROWS];
#pragma unroll
  for (int b = 0; b < NB; ++b)
#pragma unroll
    for (int r = 0; r < ROWS; ++r) acc[b][r] = 0.f;
  // thread t < NB * ROWS of a group's first wave finishes (lane t / ROWS, row t % ROWS); its residual is requested up front, its
  // latency hides under the weight stream
  const int eb = min(lane / ROWS, NB - 1), er = lane % ROWS;
  const bf16_t epi_raw = residual[(size_t)eb * ldr + min(n0 + er, N - 1)];
  for (int base = k_lo; base < k_hi; base += PRE * 2048) {
    u32x4_t xv[PRE][NB][4], wv[PRE][ROWS];
    unsigned sv[PRE][ROWS];
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
      const int c = base + it * 2048 + lane * 32;
      const int cc = c < k_hi ? c : k_lo;                    // clamped (valid) address; its product is masked out
#pragma unroll
      for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int i = 0; i < 4; ++i) xv[it][b][i] = *reinterpret_cast<const u32x4_t*>(x + (size_t)b * ldx + cc + 8 * i);
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
        float wf[ROWS][16];
#pragma unroll
        for (int r = 0; r < ROWS; ++r) cvt16_fp4(wv[it][r][2 * h], wv[it][r][2 * h + 1], s[r], wf[r]);
#pragma unroll
        for (int b = 0; b < NB; ++b) {
          float lo[8], hi[8], xf[16];
          unpack8(xv[it][b][2 * h], lo);
          unpack8(xv[it][b][2 * h + 1], hi);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            xf[i] = in ? lo[i] : 0.f;
            xf[8 + i] = in ? hi[i] : 0.f;
          }
#pragma unroll
          for (int r = 0; r < ROWS; ++r) acc[b][r] = dot16f4(wf[r], xf, acc[b][r]);
        }
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
  y[(size_t)eb * ldy + n] = resid_tail(s, epi_raw);
}

// ================================================================ launchers
// codes: K / 2 bytes per row at a 16-B aligned stride; scales: K / 32 bytes per row, contiguous (fp4_k_ok of decode_fp4.hip)
static inline bool decb4_k_ok(int B, int K, int ldx, int ldw) {
  return B >= 1 && B <= 4 && K > 0 && K % 32 == 0 && ldx >= K && ldx % 8 == 0 && ldw >= K / 2 && ldw % 16 == 0;
}
// the fused kernels: the NB staged rows fit the 64 KB of LDS a workgroup gets without opting in, less the kernels' own static
// reduction array: B * K * 2 may reach 65536 - 256 (the cap of decb8_ok, decode_batch_fp8.hip)
static inline bool decb4_ok(int B, int K, int ldx, int ldw) { return decb4_k_ok(B, K, ldx, ldw) && K <= 8192 && B * K * 2 <= 65536 - 256; }

// (PRE, XC) by row length, as DEC4_DISPATCH of decode_fp4.hip
#define DECB4_K(KERNEL, NB, K, ...)                                         \
  do {                                                                      \
    if ((K) <= 2048) KERNEL<NB, 1, 1> __VA_ARGS__;                          \
    else if ((K) <= 4096) KERNEL<NB, 2, 2> __VA_ARGS__;                     \
    else KERNEL<NB, 2, 4> __VA_ARGS__;                                      \
  } while (0)
// the residual GEMV with PRE = P12 at one and two lanes, P34 at three and four
#define DECB4_GEMV(B, ROWS, KW, P12, P34, ...) DECB_SWITCH_NB(B, decb_gemv_fp4_kernel<NB, ROWS, KW, (NB <= 2 ? P12 : P34)> __VA_ARGS__)

extern "C" int svlm_decb_qkv_fp4(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W4, int ldw,
                                 const void* w_scale, const void* bias, void* q_out, int ldq, int layer, int K, int qd, int kd, int D,
                                 void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb4_ok(B, K, ldx, ldw) && w_scale != nullptr,
                 "svlm_decb_qkv_fp4: bad B=%d K=%d ldx=%d ldw=%d (B 1..4, K a multiple of 32, ldw >= K / 2 a multiple of 16, B*K*2 <= 64 KB - 256) or no scales",
                 B, K, ldx, ldw);
  if (!decb_qkv_args_ok("svlm_decb_qkv_fp4", qd, kd, D, bias, ldq, layer)) return SVLM_EINVAL;
  const int N = qd + 2 * kd;
  DECB_SWITCH_NB(B, DECB4_K(decb_qkv_fp4_kernel, NB, K, <<<(N + 3) / 4, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const fp4x2_t*)W4, ldw, (const e8m0_t*)w_scale,
      (const bf16_t*)bias, (bf16_t*)q_out, ldq, layer, N, K, qd, kd, D)));
  return svlm_check_launch("svlm_decb_qkv_fp4");
}

extern "C" int svlm_decb_gate_up_fp4(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W4, int ldw,
                                     const void* w_scale, void* h, int ldh, int I, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb4_ok(B, K, ldx, ldw) && w_scale != nullptr && I > 0 && ldh >= I,
                 "svlm_decb_gate_up_fp4: bad B=%d I=%d K=%d ldx=%d ldw=%d ldh=%d or no scales", B, I, K, ldx, ldw, ldh);
  DECB_SWITCH_NB(B, DECB4_K(decb_gate_up_fp4_kernel, NB, K, <<<(I + 3) / 4, 256, B * K * 2, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const fp4x2_t*)W4, ldw, (const e8m0_t*)w_scale, (bf16_t*)h,
      ldh, I, K)));
  return svlm_check_launch("svlm_decb_gate_up_fp4");
}

extern "C" int svlm_decb_gemv_fp4(const void* lanes, int B, const void* x, int ldx, const void* W4, int ldw, const void* w_scale,
                                  const void* residual, int ldr, void* y, int ldy, int N, int K, void* stream) {
  SVLM_CHECK_ARG(lanes != nullptr && decb4_k_ok(B, K, ldx, ldw) && N > 0 && w_scale != nullptr,
                 "svlm_decb_gemv_fp4: bad shape B=%d N=%d K=%d ldw=%d ldx=%d (K a multiple of 32, ldw >= K / 2 a multiple of 16) or no scales", B, N,
                 K, ldw, ldx);
  SVLM_CHECK_ARG(residual != nullptr && y != nullptr && ldr >= N && ldy >= N, "svlm_decb_gemv_fp4: residual and y are required (ldr=%d ldy=%d)",
                 ldr, ldy);
  hipStream_t s = (hipStream_t)stream;
#define DECB4_GEMV_ARGS (const svlm_lane*)lanes, (const bf16_t*)x, ldx, (const fp4x2_t*)W4, ldw, (const e8m0_t*)w_scale, (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, N, K
  // the dispatch of svlm_gemv_fp4, branch for branch (ROWS, KW and the grid; PRE does not enter a row's arithmetic).  The x vectors
  // (PRE x NB x 64 B per thread) cost the occupancy, so only the one- and two-lane forms keep two K-steps in flight
  if (N <= 8192 && K >= 4096) {
    DECB4_GEMV(B, 2, 4, 2, 1, <<<(N + 1) / 2, 256, 0, s>>>(DECB4_GEMV_ARGS));
  } else if (N >= 4096 || (long long)N * K >= (8LL << 20)) {
    if (K <= 2048) DECB4_GEMV(B, 2, 1, 1, 1, <<<(N + 7) / 8, 256, 0, s>>>(DECB4_GEMV_ARGS));
    else DECB4_GEMV(B, 2, 1, 2, 1, <<<(N + 7) / 8, 256, 0, s>>>(DECB4_GEMV_ARGS));
  } else {
    if (K <= 2048) DECB4_GEMV(B, 1, 1, 1, 1, <<<(N + 3) / 4, 256, 0, s>>>(DECB4_GEMV_ARGS));
    else DECB4_GEMV(B, 1, 1, 2, 1, <<<(N + 3) / 4, 256, 0, s>>>(DECB4_GEMV_ARGS));
  }
#undef DECB4_GEMV_ARGS
  return svlm_check_launch("svlm_decb_gemv_fp4");
}
