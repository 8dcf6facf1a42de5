// Token choice with HF's logits processors, fused with the device-side token feedback that
// lets a whole decode step replay from a HIP graph without a host round trip.
//
// Reference: generate/streaming_generate_qwen.py:73-109 -- fp32 copy of the last logits row (:73),
// logits processors (:75; RepetitionPenaltyLogitsProcessor over the FULL current ids:
// score<0 ? score*p : score/p; then the warpers HF builds from the generation config: temperature,
// top-k, top-p), then argmax (:99) or softmax + multinomial (:95-97, the reference's DEFAULT:
// do_sample=True at inference.py:446), cat to input_ids (:104).
//
// Sampling on the device: plain temperature sampling is the Gumbel-max trick -- argmax_i(s_i / T + g_i) with iid standard
// Gumbel noise g_i is an exact draw from softmax(s / T) -- so it rides in the argmax kernels the greedy path already has;
// top-k / top-p go through one single-workgroup kernel (radix select of the k-th score, bitonic sort of the survivors,
// nucleus cut, inverse-CDF draw).  Noise comes from Philox4x32-10 keyed by a per-call seed in device memory and counted by
// (generated-token index, vocabulary index), so a captured graph replays fresh noise at every step.
#include "common.h"
#include "dec_sample.h"

// seen[v] = 1 for every id in ids[0..n)
__global__ void mark_seen_kernel(const int* __restrict__ ids, int n, unsigned char* __restrict__ seen, int V) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int t = ids[i];
    if (t >= 0 && t < V) seen[t] = 1;
  }
}

// Stage 1: AM_BLOCKS workgroups scan disjoint slices of the (penalised, suppressed) logits and leave
// one (value, index) candidate each in `part`.  Stage 2 (one wave) picks the winner (lowest index on
// ties, like torch.argmax) and does the device-side token feedback:
// state[0] = kv_len, state[1] = cur (index in tok_buf of the token fed to the current forward; -1 during
// prefill).  Writes tok_buf[cur+1] = argmax, marks it seen, cur += 1, kv_len += advance_kv.
#define AM_BLOCKS 64

__global__ __launch_bounds__(256) void argmax_stage1_kernel(const float* __restrict__ logits, int V,
                                                            const unsigned char* __restrict__ seen, float penalty,
                                                            const int* __restrict__ suppress, int n_suppress,
                                                            float* __restrict__ part_val, int* __restrict__ part_idx,
                                                            float inv_temp, const unsigned* __restrict__ rng,
                                                            const int* __restrict__ state) {
  const unsigned step = rng ? (unsigned)(state[1] + 1) : 0u;          // index of the token being chosen
  const int per = (V + AM_BLOCKS - 1) / AM_BLOCKS;
  const int lo = blockIdx.x * per, hi = min(V, lo + per);
  int sup[8];
#pragma unroll
  for (int s = 0; s < 8; ++s) sup[s] = s < n_suppress ? suppress[s] : -1;
  float best = -INFINITY;
  int bi = 0x7fffffff;
  for (int v = lo + threadIdx.x; v < hi; v += 256) {
    float x = logits[v];
    if (seen && seen[v]) x = x < 0.f ? x * penalty : x / penalty;
#pragma unroll
    for (int s = 0; s < 8; ++s)
      if (sup[s] == v) x = -INFINITY;
    if (rng) x = x * inv_temp + svlm_gumbel_noise(rng, step, (unsigned)v);
    am_better(best, bi, x, v);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    am_better(best, bi, ob, oi);
  }
  __shared__ float sb[4];
  __shared__ int si[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { sb[wave] = best; si[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) am_better(best, bi, sb[w], si[w]);
    part_val[blockIdx.x] = best;
    part_idx[blockIdx.x] = bi;
  }
}

__global__ __launch_bounds__(64) void argmax_stage2_kernel(const float* __restrict__ part_val, const int* __restrict__ part_idx,
                                                           unsigned char* seen, int* tok_buf, int* state, int advance_kv) {
  float best = part_val[threadIdx.x];
  int bi = part_idx[threadIdx.x];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    am_better(best, bi, ob, oi);
  }
  if (threadIdx.x == 0) {
    if (bi == 0x7fffffff) bi = 0;  // all -inf / NaN row: mirror torch.argmax's index 0
    const int cur = state[1] + 1;
    tok_buf[cur] = bi;
    state[1] = cur;
    state[0] += advance_kv;
    if (seen) seen[bi] = 1;
  }
}

extern "C" int svlm_mark_seen(const int* ids, int n, void* seen, int V, void* stream) {
  SVLM_CHECK_ARG(n >= 0 && V > 0, "svlm_mark_seen: bad n=%d V=%d", n, V);
  if (n == 0) return SVLM_OK;
  mark_seen_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(ids, n, (unsigned char*)seen, V);
  return svlm_check_launch("svlm_mark_seen");
}

extern "C" long long svlm_argmax_ws_bytes(void) { return AM_BLOCKS * 8; }

extern "C" int svlm_penalty_argmax(const float* logits, int V, void* seen, float penalty, const int* suppress, int n_suppress,
                                   int* tok_buf, int* state, int advance_kv, void* ws, void* stream) {
  SVLM_CHECK_ARG(V > 0 && penalty > 0.f && n_suppress >= 0 && n_suppress <= 8, "svlm_penalty_argmax: bad V=%d penalty=%f n_suppress=%d", V, penalty, n_suppress);
  SVLM_CHECK_ARG(ws != nullptr, "svlm_penalty_argmax: workspace of svlm_argmax_ws_bytes() bytes required");
  float* pv = (float*)ws;
  int* pi = (int*)(pv + AM_BLOCKS);
  argmax_stage1_kernel<<<AM_BLOCKS, 256, 0, (hipStream_t)stream>>>(logits, V, (const unsigned char*)seen, penalty, suppress, n_suppress, pv, pi,
                                                                   1.0f, nullptr, nullptr);
  int rc = svlm_check_launch("svlm_penalty_argmax(stage1)");
  if (rc) return rc;
  argmax_stage2_kernel<<<1, 64, 0, (hipStream_t)stream>>>(pv, pi, (unsigned char*)seen, tok_buf, state, advance_kv);
  return svlm_check_launch("svlm_penalty_argmax(stage2)");
}

// ---------------------------------------------------------------- top-k / top-p sampling (one workgroup): the bodies live in dec_sample.h
__global__ __launch_bounds__(SF_THREADS) void sample_filtered_kernel(const float* __restrict__ logits, int V,
                                                                      const unsigned char* __restrict__ seen, float penalty,
                                                                      const int* __restrict__ suppress, int n_suppress, float inv_temp,
                                                                      int top_k, float top_p, const unsigned* __restrict__ rng,
                                                                      unsigned char* seen_w, int* tok_buf, int* state, int advance_kv) {
  sample_filtered_body(logits, V, seen, penalty, suppress, n_suppress, inv_temp, top_k, top_p, rng, seen_w, tok_buf, state, advance_kv);
}

__global__ __launch_bounds__(SF_THREADS) void sample_nucleus_kernel(const float* __restrict__ logits, int V,
                                                                     const unsigned char* __restrict__ seen, float penalty,
                                                                     const int* __restrict__ suppress, int n_suppress, float inv_temp,
                                                                     int top_k, float top_p, const unsigned* __restrict__ rng,
                                                                     unsigned char* seen_w, int* tok_buf, int* state, int advance_kv) {
  sample_nucleus_body(logits, V, seen, penalty, suppress, n_suppress, inv_temp, top_k, top_p, rng, seen_w, tok_buf, state, advance_kv);
}

extern "C" int svlm_penalty_sample(const float* logits, int V, void* seen, float penalty, const int* suppress, int n_suppress,
                                   float temperature, int top_k, float top_p, const unsigned* rng, int* tok_buf, int* state,
                                   int advance_kv, void* ws, void* stream) {
  SVLM_CHECK_ARG(V > 0 && penalty > 0.f && n_suppress >= 0 && n_suppress <= 8, "svlm_penalty_sample: bad V=%d penalty=%f n_suppress=%d", V, penalty, n_suppress);
  SVLM_CHECK_ARG(temperature > 0.f && top_k >= 0 && top_p > 0.f && top_p <= 1.f && rng != nullptr && ws != nullptr,
                 "svlm_penalty_sample: bad temperature=%f top_k=%d top_p=%f", temperature, top_k, top_p);
  hipStream_t st = (hipStream_t)stream;
  if (top_k == 1) {                                    // one survivor: the argmax
    return svlm_penalty_argmax(logits, V, seen, penalty, suppress, n_suppress, tok_buf, state, advance_kv, ws, stream);
  }
  if (top_k == 0 && top_p >= 1.f) {                    // plain temperature sampling: Gumbel-max in the argmax kernels
    float* pv = (float*)ws;
    int* pi = (int*)(pv + AM_BLOCKS);
    argmax_stage1_kernel<<<AM_BLOCKS, 256, 0, st>>>(logits, V, (const unsigned char*)seen, penalty, suppress, n_suppress, pv, pi,
                                                     1.0f / temperature, rng, state);
    int rc = svlm_check_launch("svlm_penalty_sample(stage1)");
    if (rc) return rc;
    argmax_stage2_kernel<<<1, 64, 0, st>>>(pv, pi, (unsigned char*)seen, tok_buf, state, advance_kv);
    return svlm_check_launch("svlm_penalty_sample(stage2)");
  }
  if (top_k == 0 || top_k >= SF_CAP) {                 // the survivors of top-p alone (or of a very wide k) are not bounded: threshold form
    sample_nucleus_kernel<<<1, SF_THREADS, 0, st>>>(logits, V, (const unsigned char*)seen, penalty, suppress, n_suppress, 1.0f / temperature,
                                                    top_k, top_p, rng, (unsigned char*)seen, tok_buf, state, advance_kv);
    return svlm_check_launch("svlm_penalty_sample(nucleus)");
  }
  sample_filtered_kernel<<<1, SF_THREADS, 0, st>>>(logits, V, (const unsigned char*)seen, penalty, suppress, n_suppress, 1.0f / temperature,
                                                   top_k, top_p, rng, (unsigned char*)seen, tok_buf, state, advance_kv);
  return svlm_check_launch("svlm_penalty_sample(filtered)");
}
