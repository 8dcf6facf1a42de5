// The epilogue pieces of the decode-step kernels, written once: where the new token's K / V values go (all seven qkv kernels), how an
// lm_head logit becomes a candidate score and how candidates compare (all five lm_head kernels), and the residual tail of the
// lane-batched GEMVs.  The kernel shells that call them are in dec_shell.h (VALU dot products: decode_fused / _fp8 / _fp4 and
// decode_batch / _fp8 / _fp4 .hip) and in decode_wide.hip (MFMA tiles).
#pragma once
#include "common.h"

// ---------------------------------------------------------------- KV append
// Column j = n - qd of the qkv output ([k | v], kd columns each) of the token at logical row `row`, pool slot `slot`.
//   pool planes   k_planes / v_planes [Hkv][n_slots][D] of the layer: the value at (head, slot), the key UN-rotated
//                 (StreamingCache.update, streaming_cache.py:72-73)
//   linear planes k_lin / v_lin (optional, together) [Hkv][lin_rows][D] of the layer, read by svlm_decode_attn_lin without a slot
//                 table: the value row-major at logical row `row`; the key UN-rotated in its TILE position (rows at or above *lin_state
//                 are rotated by the reader).  A key tile is 16 rows x 128 dims = 2048 elements, stored as 4 groups of 32 dims; inside
//                 a group the 8-element (16-B) chunk c = (d >> 3) & 3 of tile row r = row & 15 is the 16-B unit c * 16 + r: the layout
//                 svlm_decode_attn_lin reads.  head_dim 128 only (the entries check it).
__device__ __forceinline__ void kv_append(bf16_t* k_planes, bf16_t* v_planes, int n_slots, bf16_t* k_lin, bf16_t* v_lin, int lin_rows, int row,
                                          int slot, int j, int kd, int D, bf16_t v) {
  const int jj = j < kd ? j : j - kd;
  const int h = jj / D, d = jj % D;
  bf16_t* plane = j < kd ? k_planes : v_planes;
  plane[((size_t)h * n_slots + slot) * D + d] = v;
  if (k_lin != nullptr) {
    if (j < kd) k_lin[((size_t)h * (lin_rows >> 4) + (row >> 4)) * 2048 + (d >> 5) * 512 + (((d >> 3) & 3) * 16 + (row & 15)) * 8 + (d & 7)] = v;
    else v_lin[((size_t)h * lin_rows + row) * D + d] = v;
  }
}

// ---------------------------------------------------------------- lm_head candidates
// The candidate score of vocabulary row n from its rounded logit v: repetition penalty on the tokens seen, suppression, and -- with
// rng -- temperature sampling as Gumbel-max over the processed scores (sampling.hip; every lane of a wave draws the same noise).
// state = {kv_len, cur} is read only with rng.
__device__ __forceinline__ float cand_score(float v, int n, const unsigned char* seen, float penalty,
                                            const int* suppress, int n_suppress, const unsigned* rng, float inv_temp,
                                            const int* state) {
  if (seen && seen[n]) v = v < 0.f ? v * penalty : v / penalty;
  for (int s = 0; s < n_suppress; ++s)
    if (suppress[s] == n) v = -INFINITY;
  if (rng) v = v * inv_temp + svlm_gumbel_noise(rng, (unsigned)(state[1] + 1), (unsigned)n);
  return v;
}

// (best, bi) becomes candidate (v, n) if that is better: the higher score, on a tie the lower index
__device__ __forceinline__ void cand_take(float& best, int& bi, float v, int n) {
  if (v > best || (v == best && n < bi)) { best = v; bi = n; }
}

// The workgroup's candidate per stream lane out of its four waves' (256 threads, every thread calls): on return thread b < NB holds lane
// b's winner in (bb, ii) and gets true.  The single-row kernels are the NB = 1 case.
template <int NB>
__device__ __forceinline__ bool cand_reduce(const float (&best)[NB], const int (&bi)[NB], float& bb, int& ii) {
  __shared__ float sb[NB][4];
  __shared__ int si[NB][4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) {
#pragma unroll
    for (int b = 0; b < NB; ++b) { sb[b][wave] = best[b]; si[b][wave] = bi[b]; }
  }
  __syncthreads();
  if (threadIdx.x >= NB) return false;
  const int b = threadIdx.x;
  bb = sb[b][0];
  ii = si[b][0];
  for (int w = 1; w < 4; ++w) cand_take(bb, ii, sb[b][w], si[b][w]);
  return true;
}

// ---------------------------------------------------------------- residual tail of the lane-batched GEMVs
// y = bf16(bf16(s) + residual).  The "+ 0.f" is the single-row kernels' "+ no bias": -0 becomes +0 there too.
__device__ __forceinline__ bf16_t resid_tail(float s, bf16_t residual) {
  float v = rbf(s + 0.f);
  v = rbf(v + bf2f(residual));
  return f2bf(v);
}
