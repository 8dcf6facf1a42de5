// e4m3 weight-stream pieces shared by the single-row (decode_fp8.hip) and the lane-batched (decode_batch_fp8.hip) fp8 decode
// kernels: the activation fetch of one lane's K-step, the 16-element dot product in element order, the pre-issued head of a
// wave's weight rows, and the format policy WFp8 of the kernel shells (dec_shell.h).  A K-step is 1024 elements, 16 consecutive ones
// per thread (one 16-B load = 16 codes).  x16 and f32x2_t also serve the fp4 kernels (dec_fp4.h).
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef uint8_t fp8_t;

// the 16 bf16 activations of one lane's K-step, as fp32 (zero past K)
__device__ __forceinline__ void x16(const bf16_t* xs, int c, int K, float (&xf)[16]) {
  const int cc = c < K ? c : 0;
  const u32x4_t a = *reinterpret_cast<const u32x4_t*>(xs + cc);
  const u32x4_t b = *reinterpret_cast<const u32x4_t*>(xs + cc + 8);
  float lo[8], hi[8];
  unpack8(a, lo);
  unpack8(b, hi);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    xf[i] = c < K ? lo[i] : 0.f;
    xf[8 + i] = c < K ? hi[i] : 0.f;
  }
}

// acc += sum_j e4m3(w byte j) * xf[j], in element order
__device__ __forceinline__ float dot16(const u32x4_t& w, const float (&xf)[16], float acc) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x2_t lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], false);
    const f32x2_t hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[i], true);
    acc = fmaf(lo[0], xf[4 * i], acc);
    acc = fmaf(lo[1], xf[4 * i + 1], acc);
    acc = fmaf(hi[0], xf[4 * i + 2], acc);
    acc = fmaf(hi[1], xf[4 * i + 3], acc);
  }
  return acc;
}

template <int NR, int PRE>
struct W8Pre {
  u32x4_t w[PRE][NR];
};
template <int NR, int PRE>
__device__ __forceinline__ void preload_w8(const fp8_t* const (&wr)[NR], int base, int K, W8Pre<NR, PRE>& pre) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 1024 + lane * 16;
    const int cc = c < K ? c : 0;                            // clamped (valid) address; its product is masked out
#pragma unroll
    for (int r = 0; r < NR; ++r) pre.w[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + cc));
  }
}

// the K loops, defined where they are used: the single-row one in decode_fp8.hip, the lane-batched one in decode_batch_fp8.hip
template <int NR, int PRE>
__device__ __forceinline__ void wave_dots8(const fp8_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NR], W8Pre<NR, PRE>& pre);
template <int NB, int NR, int PRE>
__device__ __forceinline__ void wave_dots8_b(const fp8_t* const (&wr)[NR], const bf16_t* xs, int K, float (&acc)[NB][NR], W8Pre<NR, PRE>& pre);

// format policy (see WBf16, dec_stream.h).  e4m3: a row is its code pointer; its scale S[n] is fetched by the shell with the row's
// index and multiplied in once, in the epilogue.
struct WFp8 {
  typedef fp8_t w_t;
  typedef float s_t;                  // one power-of-two scale per output row
  static constexpr bool row_scale = true;
  template <int NR>
  struct Rows {
    const fp8_t* w[NR];
  };
  template <int NR, int PRE>
  using Pre = W8Pre<NR, PRE>;
  template <int NR>
  static __device__ __forceinline__ void row(Rows<NR>& R, int r, const w_t* W, int ldw, const s_t*, int n, int) { R.w[r] = W + (size_t)n * ldw; }
  template <int NR, int PRE>
  static __device__ __forceinline__ void preload(const Rows<NR>& R, int base, int K, Pre<NR, PRE>& pre) { preload_w8<NR, PRE>(R.w, base, K, pre); }
  template <int NR, int PRE>
  static __device__ __forceinline__ void dots(const Rows<NR>& R, const bf16_t* xs, int K, float (&acc)[NR], Pre<NR, PRE>& pre) {
    wave_dots8<NR, PRE>(R.w, xs, K, acc, pre);
  }
  template <int NB, int NR, int PRE>
  static __device__ __forceinline__ void dots_b(const Rows<NR>& R, const bf16_t* xs, int K, float (&acc)[NB][NR], Pre<NR, PRE>& pre) {
    wave_dots8_b<NB, NR, PRE>(R.w, xs, K, acc, pre);
  }
};
