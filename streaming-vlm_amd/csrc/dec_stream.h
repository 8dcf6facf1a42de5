// bf16 weight-stream pieces of the decode kernels, shared by the single-row (decode_fused.hip) and the lane-batched (decode_batch.hip)
// forms: the pre-issued head of a wave's weight rows, the bf16 format policy WBf16 of the kernel shells
// (dec_shell.h), and the winner-over-candidates + token feedback of svlm_argmax_finish.
#pragma once
#include "common.h"

// The first PRE K-steps (512 elements each) of a wave's weight rows are requested BEFORE the activation row is
// normalised and staged: weights do not depend on x, so the HBM latency of the stream's head overlaps the norm.
// PRE = 3 covers the whole row at K = 1536 (Qwen2-VL-2B); longer rows continue in fully pre-issued batches of PRE.
template <int NR, int PRE>
struct WPre {
  u32x4_t w[PRE][NR];
};
template <int NR, int PRE>
__device__ __forceinline__ void preload_w(const bf16_t* const (&wr)[NR], int base, int K, WPre<NR, PRE>& pre) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 512 + lane * 8;
    const int cc = c < K ? c : 0;                            // clamped (valid) address; its product is masked out
#pragma unroll
    for (int r = 0; r < NR; ++r) pre.w[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + cc));
  }
}

// The K loops of the bf16 weight stream, defined where they are used: the single-row one in decode_fused.hip, the lane-batched one in
// decode_batch.hip.
template <int NR, int PRE>
__device__ __forceinline__ void wave_dots(const bf16_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NR], WPre<NR, PRE>& pre);
template <int NB, int NR, int PRE>
__device__ __forceinline__ void wave_dots_b(const bf16_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NB][NR], WPre<NR, PRE>& pre);

// WEIGHT-FORMAT POLICY of the kernel shells (dec_shell.h).  A policy only NAMES what a format has -- the kernel-argument types, the
// handles of a wave's NR rows, the pre-issued registers, the preload and the two K loops -- and has no arithmetic of its own.
// bf16: a row is its pointer; no scale.
struct WBf16 {
  typedef bf16_t w_t;                 // the weight argument
  typedef void s_t;                   // the scale argument (none)
  static constexpr bool row_scale = false;
  template <int NR>
  struct Rows {
    const bf16_t* w[NR];
  };
  template <int NR, int PRE>
  using Pre = WPre<NR, PRE>;
  template <int NR>
  static __device__ __forceinline__ void row(Rows<NR>& R, int r, const w_t* W, int ldw, const s_t*, int n, int) { R.w[r] = W + (size_t)n * ldw; }
  template <int NR, int PRE>
  static __device__ __forceinline__ void preload(const Rows<NR>& R, int base, int K, Pre<NR, PRE>& pre) { preload_w<NR, PRE>(R.w, base, K, pre); }
  template <int NR, int PRE>
  static __device__ __forceinline__ void dots(const Rows<NR>& R, const bf16_t* xs, int K, float (&acc)[NR], Pre<NR, PRE>& pre) {
    wave_dots<NR, PRE>(R.w, xs, K, acc, pre);
  }
  template <int NB, int NR, int PRE>
  static __device__ __forceinline__ void dots_b(const Rows<NR>& R, const bf16_t* xs, int K, float (&acc)[NB][NR], Pre<NR, PRE>& pre) {
    wave_dots_b<NB, NR, PRE>(R.w, xs, K, acc, pre);
  }
};

// winner over the per-workgroup candidates of a dec_lm_head launch + device-side token feedback; one 1024-thread workgroup
__device__ __forceinline__ void argmax_finish_body(const float* __restrict__ part_val, const int* __restrict__ part_idx, int n_parts,
                                                   unsigned char* seen, int* tok_buf, int* state, int advance_kv) {
  float best = -INFINITY;
  int bi = 0x7fffffff;
  // the candidates are the output of the launch in front: every load here is a round trip to another CU's stores (~2 us each behind a
  // kernel boundary), so ALL of them are requested before the first compare -- 16-B loads, six per thread (24k candidates), the rest
  // (a vocabulary beyond 196k, an unaligned tail) in the plain loop
  constexpr int VL = 6;
  const int n4 = ((reinterpret_cast<uintptr_t>(part_val) | reinterpret_cast<uintptr_t>(part_idx)) & 15) == 0 ? n_parts >> 2 : 0;
  f32x4_t vv[VL];
  typedef int i32x4_t __attribute__((ext_vector_type(4)));
  i32x4_t vi[VL];
  if (n4 > 0) {                     // (kernel-uniform)
#pragma unroll
    for (int u = 0; u < VL; ++u) {
      const int j = min((int)threadIdx.x + u * 1024, n4 - 1);
      vv[u] = reinterpret_cast<const f32x4_t*>(part_val)[j];
      vi[u] = reinterpret_cast<const i32x4_t*>(part_idx)[j];
    }
  }
#pragma unroll
  for (int u = 0; u < VL; ++u) {
    if ((int)threadIdx.x + u * 1024 < n4) {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float v = vv[u][e];
        const int n = vi[u][e];
        if (v > best || (v == best && n < bi)) { best = v; bi = n; }
      }
    }
  }
#pragma unroll 4
  for (int i = min(n4, VL * 1024) * 4 + threadIdx.x; i < n_parts; i += 1024) {
    const float v = part_val[i];
    const int n = part_idx[i];
    if (v > best || (v == best && n < bi)) { best = v; bi = n; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  __shared__ float sb[16];
  __shared__ int si[16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (lane == 0) { sb[wave] = best; si[wave] = bi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 16; ++w)
      if (sb[w] > best || (sb[w] == best && si[w] < bi)) { best = sb[w]; bi = si[w]; }
    if (bi == 0x7fffffff) bi = 0;
    const int cur = state[1] + 1;
    tok_buf[cur] = bi;
    state[1] = cur;
    state[0] += advance_kv;
    if (seen) seen[bi] = 1;
  }
}
