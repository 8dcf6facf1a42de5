// MXFP4 weight-stream pieces shared by the single-row (decode_fp4.hip) and the lane-batched (decode_batch_fp4.hip) fp4 decode kernels,
// with the format policy WFp4 of the kernel shells (dec_shell.h): OCP e2m1 codes, two per byte (element 2i in the low nibble of
// byte i), one e8m0 scale byte per block of 32 consecutive K elements in an array of its own (row-major, K / 32 per row).  A K-step is
// 2048 elements, 32 consecutive ones per lane: one 16-B load = 32 codes = exactly one block, so a lane needs one scale byte per load.
#pragma once
#include "common.h"
#include "dec_fp8.h"              // x16, f32x2_t

typedef uint8_t fp4x2_t;          // two e2m1 codes
typedef uint8_t e8m0_t;           // scale byte b: 2^(b - 127)

// the scale as the float the conversion multiplies with: a normal fp32 for every byte in [1, 254]
__device__ __forceinline__ float e8m0_f32(unsigned b) { return __uint_as_float(b << 23); }

// acc += sum_j e2m1(code j of w0 | w1) * s * xf[j], j = 0..15 in element order.  v_cvt_scalef32_pk_f32_fp4 turns one byte (two codes,
// low nibble first) into two fp32 already multiplied by s: exact, s being a power of two and a code having 2 significant bits.
__device__ __forceinline__ float dot16_fp4(unsigned w0, unsigned w1, float s, const float (&xf)[16], float acc) {
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const unsigned w = h ? w1 : w0;
    const f32x2_t a = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 0);
    const f32x2_t b = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 1);
    const f32x2_t c = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 2);
    const f32x2_t d = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(w, s, 3);
    acc = fmaf(a[0], xf[8 * h], acc);
    acc = fmaf(a[1], xf[8 * h + 1], acc);
    acc = fmaf(b[0], xf[8 * h + 2], acc);
    acc = fmaf(b[1], xf[8 * h + 3], acc);
    acc = fmaf(c[0], xf[8 * h + 4], acc);
    acc = fmaf(c[1], xf[8 * h + 5], acc);
    acc = fmaf(d[0], xf[8 * h + 6], acc);
    acc = fmaf(d[1], xf[8 * h + 7], acc);
  }
  return acc;
}

// PRE K-steps of NR rows in flight: per (K-step, row) one 16-B load of codes and one scale byte
template <int NR, int PRE>
struct W4Pre {
  u32x4_t w[PRE][NR];
  unsigned s[PRE][NR];
};
// wr[r] / sr[r]: the row's codes and scale bytes; K / 32 blocks per row
template <int NR, int PRE>
__device__ __forceinline__ void preload_w4(const fp4x2_t* const (&wr)[NR], const e8m0_t* const (&sr)[NR], int base, int K,
                                           W4Pre<NR, PRE>& pre) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
    const int c = base + it * 2048 + lane * 32;
    const int cc = c < K ? c : 0;                            // clamped (valid) address; its product is masked out
#pragma unroll
    for (int r = 0; r < NR; ++r) {
      pre.w[it][r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wr[r] + (cc >> 1)));
      pre.s[it][r] = sr[r][cc >> 5];
    }
  }
}

// the K loops, defined where they are used: the single-row one in decode_fp4.hip, the lane-batched one in decode_batch_fp4.hip
template <int NR, int PRE>
__device__ __forceinline__ void wave_dots4(const fp4x2_t* const (&wr)[NR], const e8m0_t* const (&sr)[NR], const bf16_t* xs, int K,
                                           float (&acc)[NR], W4Pre<NR, PRE>& pre);
template <int NB, int NR, int PRE>
__device__ __forceinline__ void wave_dots4_b(const fp4x2_t* const (&wr)[NR], const e8m0_t* const (&sr)[NR], const bf16_t* xs, int K,
                                             float (&acc)[NB][NR], W4Pre<NR, PRE>& pre);

// format policy (see WBf16, dec_stream.h).  MXFP4: a row is its code pointer plus the pointer to its K / 32 scale bytes; the scales
// are applied inside the K loop's conversion, so there is no row scale.
struct WFp4 {
  typedef fp4x2_t w_t;
  typedef e8m0_t s_t;
  static constexpr bool row_scale = false;
  template <int NR>
  struct Rows {
    const fp4x2_t* w[NR];
    const e8m0_t* s[NR];
  };
  template <int NR, int PRE>
  using Pre = W4Pre<NR, PRE>;
  template <int NR>
  static __device__ __forceinline__ void row(Rows<NR>& R, int r, const w_t* W, int ldw, const s_t* S, int n, int K) {
    R.w[r] = W + (size_t)n * ldw;
    R.s[r] = S + (size_t)n * (K >> 5);
  }
  template <int NR, int PRE>
  static __device__ __forceinline__ void preload(const Rows<NR>& R, int base, int K, Pre<NR, PRE>& pre) {
    preload_w4<NR, PRE>(R.w, R.s, base, K, pre);
  }
  template <int NR, int PRE>
  static __device__ __forceinline__ void dots(const Rows<NR>& R, const bf16_t* xs, int K, float (&acc)[NR], Pre<NR, PRE>& pre) {
    wave_dots4<NR, PRE>(R.w, R.s, xs, K, acc, pre);
  }
  template <int NB, int NR, int PRE>
  static __device__ __forceinline__ void dots_b(const Rows<NR>& R, const bf16_t* xs, int K, float (&acc)[NB][NR], Pre<NR, PRE>& pre) {
    wave_dots4_b<NB, NR, PRE>(R.w, R.s, xs, K, acc, pre);
  }
};
