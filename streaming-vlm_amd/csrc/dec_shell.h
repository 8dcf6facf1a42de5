// The shells of the fused decode-step kernels, one per op, over a weight-format policy F (WBf16: dec_stream.h, WFp8: dec_fp8.h,
// WFp4: dec_fp4.h).  A shell is everything around a format's K loop: row handles, the activation prologue (dec_xrow.h / dec_lanes.h),
// the pre-issued head of the weight stream, the bounds return, F's K loop, and the lane-0 epilogue built from dec_epi.h.  The
// fused __global__ kernels of decode_fused / _fp8 / _fp4 .hip (single-row) and decode_batch / _fp8 / _fp4 .hip (lane-batched) are one-line
// calls of these (but the lane-batched e4m3 head, which keeps a body of its own in decode_batch_fp8.hip).  A new weight format is a policy plus its K loops; nothing here changes.
//
// A format with one scale per output row (F::row_scale, fp8) has the scale fetched with the pre-issued loads and multiplied in once,
// in the epilogue; the other formats get neither the load nor the multiply.
#pragma once
#include "common.h"
#include "dec_xrow.h"
#include "dec_lanes.h"
#include "dec_epi.h"

template <typename F>
__device__ __forceinline__ float w_scale_of(const typename F::s_t* __restrict__ S, int n) {
  if constexpr (F::row_scale) return S[n];
  else return 1.f;
}
template <typename F>
__device__ __forceinline__ float w_scaled(float acc, float s) {
  if constexpr (F::row_scale) return acc * s;
  else return acc;
}

// ================================================================ single-row shells: ROWS output rows per wave, 4 waves
// ---------------------------------------------------------------- QKV + KV append
template <typename F, int ROWS, int PRE, int XC>
__device__ __forceinline__ void dec_qkv_body(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                             const typename F::w_t* __restrict__ W, int ldw, const typename F::s_t* __restrict__ S,
                                             const bf16_t* __restrict__ bias, bf16_t* __restrict__ q_out, bf16_t* __restrict__ k_planes,
                                             bf16_t* __restrict__ v_planes, const int* __restrict__ slot_of, const int* __restrict__ len_dev,
                                             int len_host, int N, int K, int qd, int kd, int D, int n_slots, bf16_t* __restrict__ k_lin,
                                             bf16_t* __restrict__ v_lin, int lin_rows) {
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  typename F::template Rows<ROWS> wr;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) F::row(wr, r, W, ldw, S, min(n0 + r, N - 1), K);
  // x first, then everything that does not depend on it: head of the weight stream, the slot, the bias, the scale
  XRow<XC> xr;
  load_x<XC>(x, ln_w, K, xr);
  __builtin_amdgcn_sched_barrier(0);
  typename F::template Pre<ROWS, PRE> pre;
  F::template preload<ROWS, PRE>(wr, 0, K, pre);
  const int row = len_dev ? *len_dev : len_host;
  const int slot = slot_of[row];
  bf16_t bpre[ROWS];
  float spre[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    bpre[r] = bias[min(n0 + r, N - 1)];
    spre[r] = w_scale_of<F>(S, min(n0 + r, N - 1));
  }
  __builtin_amdgcn_sched_barrier(0);
  stage_x<XC>(xr, eps, K, xs);
  if (n0 >= N) return;
  float acc[ROWS];
  F::template dots<ROWS, PRE>(wr, xs, K, acc, pre);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = n0 + r;
      if (n >= N) break;
      const bf16_t v = f2bf(w_scaled<F>(acc[r], spre[r]) + bf2f(bpre[r]));
      if (n < qd) q_out[n] = v;
      else kv_append(k_planes, v_planes, n_slots, k_lin, v_lin, lin_rows, row, slot, n - qd, kd, D, v);
    }
  }
}

// ---------------------------------------------------------------- gate/up + SwiGLU
template <typename F, int ROWS, int PRE, int XC>
__device__ __forceinline__ void dec_gate_up_body(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                 const typename F::w_t* __restrict__ W, int ldw, const typename F::s_t* __restrict__ S,
                                                 bf16_t* __restrict__ h, int I, int K) {
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  typename F::template Rows<2 * ROWS> wr;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = min(n0 + r, I - 1);
    F::row(wr, r, W, ldw, S, n, K);                // gate row n
    F::row(wr, ROWS + r, W, ldw, S, I + n, K);     // up row n
  }
  XRow<XC> xr;
  load_x<XC>(x, ln_w, K, xr);
  __builtin_amdgcn_sched_barrier(0);
  typename F::template Pre<2 * ROWS, PRE> pre;
  F::template preload<2 * ROWS, PRE>(wr, 0, K, pre);
  float spre[2 * ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = min(n0 + r, I - 1);
    spre[r] = w_scale_of<F>(S, n);
    spre[ROWS + r] = w_scale_of<F>(S, I + n);
  }
  __builtin_amdgcn_sched_barrier(0);
  stage_x<XC>(xr, eps, K, xs);
  if (n0 >= I) return;
  float acc[2 * ROWS];
  F::template dots<2 * ROWS, PRE>(wr, xs, K, acc, pre);
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = n0 + r;
      if (n >= I) break;
      const float g = rbf(w_scaled<F>(acc[r], spre[r])), u = rbf(w_scaled<F>(acc[ROWS + r], spre[ROWS + r]));
      h[n] = f2bf(apply_act(g, SVLM_ACT_SILU) * u);
    }
  }
}

// ---------------------------------------------------------------- lm_head + penalty + argmax candidates
// logits: the fp32 copy of the bf16 value; one candidate per workgroup (4 x ROWS vocabulary rows); rng: Gumbel noise in the candidates
template <typename F, int ROWS, int PRE, int XC>
__device__ __forceinline__ void dec_lm_head_body(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, float eps,
                                                 const typename F::w_t* __restrict__ W, int ldw, const typename F::s_t* __restrict__ S,
                                                 float* __restrict__ logits, const unsigned char* __restrict__ seen, float penalty,
                                                 const int* __restrict__ suppress, int n_suppress, float* __restrict__ part_val,
                                                 int* __restrict__ part_idx, int V, int K, float inv_temp, const unsigned* __restrict__ rng,
                                                 const int* __restrict__ state) {
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  typename F::template Rows<ROWS> wr;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) F::row(wr, r, W, ldw, S, min(n0 + r, V - 1), K);
  XRow<XC> xr;
  load_x<XC>(x, ln_w, K, xr);
  __builtin_amdgcn_sched_barrier(0);
  typename F::template Pre<ROWS, PRE> pre;
  F::template preload<ROWS, PRE>(wr, 0, K, pre);
  float spre[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) spre[r] = w_scale_of<F>(S, min(n0 + r, V - 1));
  __builtin_amdgcn_sched_barrier(0);
  stage_x<XC>(xr, eps, K, xs);
  float best[1] = {-INFINITY};
  int bi[1] = {0x7fffffff};
  if (n0 < V) {
    float acc[ROWS];
    F::template dots<ROWS, PRE>(wr, xs, K, acc, pre);
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = n0 + r;
      if (n >= V) break;
      float v = rbf(w_scaled<F>(acc[r], spre[r]));
      if (lane == 0) logits[n] = v;
      v = cand_score(v, n, seen, penalty, suppress, n_suppress, rng, inv_temp, state);
      cand_take(best[0], bi[0], v, n);
    }
  }
  float bb;
  int ii;
  if (cand_reduce<1>(best, bi, bb, ii)) {      // (the 1-lane case: thread 0 holds the workgroup's candidate)
    part_val[blockIdx.x] = bb;
    part_idx[blockIdx.x] = ii;
  }
}

// ================================================================ lane-batched shells: NB stream lanes (dec_lanes.h) on one weight read
// A lane that is not live is skipped: no KV row, no output row, no candidate written.
// ---------------------------------------------------------------- QKV + KV append (one output row per wave)
template <typename F, int NB, int PRE, int XC>
__device__ __forceinline__ void decb_qkv_body(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                              const bf16_t* __restrict__ ln_w, float eps, const typename F::w_t* __restrict__ W, int ldw,
                                              const typename F::s_t* __restrict__ S, const bf16_t* __restrict__ bias,
                                              bf16_t* __restrict__ q_out, int ldq, int layer, int N, int K, int qd, int kd, int D) {
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  const int nc = min(n, N - 1);
  typename F::template Rows<1> wr;
  F::row(wr, 0, W, ldw, S, nc, K);
  XRow<XC> xr[NB];
  bool live[NB];
  load_rows<NB, XC>(lanes, x, ldx, ln_w, K, xr, live);
  __builtin_amdgcn_sched_barrier(0);
  typename F::template Pre<1, PRE> pre;
  F::template preload<1, PRE>(wr, 0, K, pre);
  const bf16_t bpre = bias[nc];
  const float spre = w_scale_of<F>(S, nc);
  __builtin_amdgcn_sched_barrier(0);
  stage_rows<NB, XC>(xr, live, eps, K, xs);
  if (n >= N) return;
  float acc[NB][1];
  F::template dots_b<NB, 1, PRE>(wr, xs, K, acc, pre);
  if (lane == 0) {
    const int Hkv = kd / D;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (!live[b]) continue;
      const svlm_lane& L = lanes[b];
      const bf16_t v = f2bf(w_scaled<F>(acc[b][0], spre) + bf2f(bpre));
      if (n < qd) {
        q_out[(size_t)b * ldq + n] = v;
      } else {
        const int row = L.state[0];
        lane_kv_append(L, layer, Hkv, D, row, L.slot_of[row], n - qd, kd, v);
      }
    }
  }
}

// ---------------------------------------------------------------- gate/up + SwiGLU (one gate row and its up row per wave)
template <typename F, int NB, int PRE, int XC>
__device__ __forceinline__ void decb_gate_up_body(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                                  const bf16_t* __restrict__ ln_w, float eps, const typename F::w_t* __restrict__ W, int ldw,
                                                  const typename F::s_t* __restrict__ S, bf16_t* __restrict__ h, int ldh, int I, int K) {
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + wave;
  const int nc = min(n, I - 1);
  typename F::template Rows<2> wr;
  F::row(wr, 0, W, ldw, S, nc, K);                 // gate row n
  F::row(wr, 1, W, ldw, S, I + nc, K);             // up row n
  XRow<XC> xr[NB];
  bool live[NB];
  load_rows<NB, XC>(lanes, x, ldx, ln_w, K, xr, live);
  __builtin_amdgcn_sched_barrier(0);
  typename F::template Pre<2, PRE> pre;
  F::template preload<2, PRE>(wr, 0, K, pre);
  const float sg = w_scale_of<F>(S, nc), su = w_scale_of<F>(S, I + nc);
  __builtin_amdgcn_sched_barrier(0);
  stage_rows<NB, XC>(xr, live, eps, K, xs);
  if (n >= I) return;
  float acc[NB][2];
  F::template dots_b<NB, 2, PRE>(wr, xs, K, acc, pre);
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      if (!live[b]) continue;
      const float g = rbf(w_scaled<F>(acc[b][0], sg)), u = rbf(w_scaled<F>(acc[b][1], su));
      h[(size_t)b * ldh + n] = f2bf(apply_act(g, SVLM_ACT_SILU) * u);
    }
  }
}

// ---------------------------------------------------------------- lm_head + penalty + argmax candidates
// ROWS = the single-row kernel's vocabulary rows per wave: the candidates are per workgroup of 4 x ROWS rows.  SMP: a live lane whose
// sampling record says Gumbel gets score * inv_temp + noise(seed, token index, vocabulary index) as its candidate score, the expression
// of the single-row kernel; the logits row and the other lanes' candidates do not change.
template <typename F, int NB, int ROWS, int PRE, int XC, bool SMP>
__device__ __forceinline__ void decb_lm_head_body(const svlm_lane* __restrict__ lanes, const svlm_lane_sample* __restrict__ samples,
                                                  const bf16_t* __restrict__ x, int ldx, const bf16_t* __restrict__ ln_w, float eps,
                                                  const typename F::w_t* __restrict__ W, int ldw, const typename F::s_t* __restrict__ S,
                                                  float* __restrict__ logits, int ldl, const int* __restrict__ suppress,
                                                  float* __restrict__ ws, long long ws_stride, int V, int K) {
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int n0 = (blockIdx.x * 4 + wave) * ROWS;
  typename F::template Rows<ROWS> wr;
#pragma unroll
  for (int r = 0; r < ROWS; ++r) F::row(wr, r, W, ldw, S, min(n0 + r, V - 1), K);
  XRow<XC> xr[NB];
  bool live[NB];
  load_rows<NB, XC>(lanes, x, ldx, ln_w, K, xr, live);
  __builtin_amdgcn_sched_barrier(0);
  typename F::template Pre<ROWS, PRE> pre;
  F::template preload<ROWS, PRE>(wr, 0, K, pre);
  float spre[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) spre[r] = w_scale_of<F>(S, min(n0 + r, V - 1));
  __builtin_amdgcn_sched_barrier(0);
  stage_rows<NB, XC>(xr, live, eps, K, xs);
  float best[NB];
  int bi[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) { best[b] = -INFINITY; bi[b] = 0x7fffffff; }
  if (n0 < V) {
    float acc[NB][ROWS];
    F::template dots_b<NB, ROWS, PRE>(wr, xs, K, acc, pre);
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
        float v = rbf(w_scaled<F>(acc[b][r], spre[r]));
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
