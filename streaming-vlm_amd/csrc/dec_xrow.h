// Activation-row prologue shared by the fused decode-step GEMVs (decode_fused.hip: bf16 weights, decode_fp8.hip: e4m3 weights):
// load the row once, RMSNorm it and stage it in LDS as bf16, rounded where the eager module rounds.
#pragma once
#include "common.h"

extern __shared__ __attribute__((aligned(16))) unsigned char dyn_smem[];

// The activation row is loaded ONCE, 8 elements per thread per chunk (XC chunks of 2048 cover K), together with the norm
// gain, BEFORE the weight preloads are issued: vmcnt retires in order, so a wait for x placed behind the weight loads
// would wait for the head of the weight stream as well.
template <int XC>
struct XRow {
  u32x4_t x[XC], g[XC];
};
template <int XC>
__device__ __forceinline__ void load_x(const bf16_t* __restrict__ x, const bf16_t* __restrict__ ln_w, int K, XRow<XC>& xr) {
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    const int c = (i * 256 + threadIdx.x) * 8;
    const int cc = c < K ? c : 0;
    xr.x[i] = *reinterpret_cast<const u32x4_t*>(x + cc);
    xr.g[i] = *reinterpret_cast<const u32x4_t*>(ln_w + cc);
  }
}

// xs[0..K) = bf16( w * bf16(x * rsqrt(mean(x^2) + eps)) ), rounded exactly where the eager module rounds.  256 threads.
// LDS-only barriers: the weight loads issued before this call stay in flight across them.
template <int XC>
__device__ __forceinline__ void stage_x(const XRow<XC>& xr, float eps, int K, bf16_t* xs) {
  __shared__ float red[4];
  const int tid = threadIdx.x;
  float f[XC][8];
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    unpack8(xr.x[i], f[i]);
    if ((i * 256 + tid) * 8 < K) {
#pragma unroll
      for (int j = 0; j < 8; ++j) ss += f[i][j] * f[i][j];
    }
  }
  ss = wave_sum(ss);
  if ((tid & 63) == 0) red[tid >> 6] = ss;
  lds_barrier();
  const float r = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
#pragma unroll
  for (int i = 0; i < XC; ++i) {
    const int c = (i * 256 + tid) * 8;
    if (c < K) {
      float g[8];
      unpack8(xr.g[i], g);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[i][j] = g[j] * rbf(f[i][j] * r);
      *reinterpret_cast<u32x4_t*>(xs + c) = pack8(f[i]);
    }
  }
  lds_barrier();
}
