// Wide lane-batched decode-step kernels: the weight GEMVs of a stream group's decode step as skinny GEMMs on the matrix cores, for
// B = 1..16 lanes.  One v_mfma_f32_16x16x32_bf16 multiplies 16 weight rows (the A operand) with the activation rows of up to 16 lanes
// (the B operand, one lane per column), so the cost of a step's weight kernels is flat in the lane count where decode_batch.hip
// (VALU dot products, every weight row times every lane's LDS row) grows with it.
//
//   svlm_decw_qkv            RMSNorm + QKV + bias + KV append, as svlm_decb_qkv
//   svlm_decw_gemv           o_proj / down_proj with residual, as svlm_decb_gemv
//   svlm_decw_gate_up        RMSNorm + gate/up + SwiGLU, as svlm_decb_gate_up
//   svlm_decw_lm_head        RMSNorm + head + penalty + suppression + argmax candidates in the workspace format of svlm_decb_lm_head
//                            (one candidate per 8 vocabulary rows), completed by the unchanged finish kernel
//   svlm_decw_embed / svlm_decw_argmax_finish   the kernels of decode_batch.hip, whose grids are one workgroup (row) per lane, for 1..16 lanes
//
// OPERANDS.  A workgroup owns one tile of 16 consecutive weight rows (gate_up: the 16 gate rows and the 16 up rows of the same outputs).
// K is walked in blocks of 64: in block b, MFMA s (s = 0, 1) of lane l (r = l & 15, g = l >> 4) takes k = 64 b + 16 g + 8 s + j,
// j = 0..7, for BOTH operands -- a permutation of k inside the block, so that a lane's two A fragments are 32 contiguous bytes of weight
// row r and the four lane groups cover one 128-B line of it.  The weights go straight from global memory to VGPRs (non-temporal 16-B
// loads, the next batch of PRE blocks requested before the current one is multiplied); no LDS.  Column c of the B operand is lane c's
// activation row; columns >= B are zero.  Columns of lanes that are not live are multiplied like the others and never written.
//
// SPLIT PLAN (svlm_decw_plan; a function of K and the entry only, never of B).  K is split over the KW waves of the workgroup in whole
// blocks: wave w takes blocks [w bpw, (w + 1) bpw), bpw = ceil(ceil(K / 64) / KW).  The fused entries have KW = 4 (the 256 threads of
// the norm prologue); svlm_decw_gemv has KW = 4 / 8 / 16 for ceil(K / 64) < 16 / < 64 / >= 64.  Every wave writes its fp32 tile to LDS
// and wave 0 adds them as part[0] + part[1] + ... + part[KW - 1]: a fixed order, no atomics.  K is not split across workgroups.
//
// NORM PROLOGUE.  The staged rows are bit for bit stage_x's (dec_xrow.h): wave w normalises rows w, w + 4, w + 8, w + 12 by itself,
// standing in for the four waves of stage_x one after the other -- the same per-thread chain over the same elements, the same
// wave_sum, the same red[0] + red[1] + red[2] + red[3] -- so no barrier is needed until all rows are staged.  Rows are padded to an
// odd number of 16-B slots (conflict-free ds_read_b128 over 16 rows).  Only rows of live lanes are staged.
//
// LANE INDEPENDENCE.  A column of the MFMA result depends on that column of the B operand alone, and neither the split plan nor a
// wave's instruction stream depends on B or on which column a lane sits in: a live lane's outputs are a function of its own inputs.
//
// EPILOGUES.  The new K / V row goes where every qkv kernel puts it (lane_kv_append, dec_lanes.h -> kv_append, dec_epi.h); the head's
// candidates are scored and compared by cand_score / cand_take and the residual GEMV ends in resid_tail (dec_epi.h), as in the VALU
// kernels.  The MFMA loops and the norm prologue are this file's own.
//
// Arguments: 1 <= B <= 16; K > 0 and a multiple of 8 (the last block is masked in 8-element chunks); leading dimensions as the
// svlm_decb_* entries.  The fused entries need K <= 4096 and B * ldxs(K) * 2 <= 120 KB of dynamic LDS (ldxs = the padded row).
#include "common.h"
#include "dec_xrow.h"
#include "dec_stream.h"
#include "dec_launch.h"           // host side: the qkv argument check
#include "dec_lanes.h"            // the lane table, lane_kv_append; the epilogue pieces shared with the VALU kernels: dec_epi.h

#define DECW_MAX_LANES 16
#define DECW_PRE 4                      // fused kernels: blocks per weight batch (two batches in registers)
#define DECW_PRE_GEMV 2                 // svlm_decw_gemv: weights and activations both come from global memory
#define DECW_LDS_DYN_MAX (120 * 1024)

static inline int decw_ldxs(int K) { return K + (((K >> 3) & 1) ? 16 : 8); }
__device__ __forceinline__ int decw_ldxs_d(int K) { return K + (((K >> 3) & 1) ? 16 : 8); }

__device__ __forceinline__ bf16x8_t as_frag(const u32x4_t& v) { return __builtin_bit_cast(bf16x8_t, v); }

// the weight fragments of PRE blocks of NT tiles: a[it][t][s], 16 B each
template <int NT, int PRE>
struct WFrag {
  u32x4_t a[PRE][NT][2];
};
// wrow[t]: this lane's weight row (row l & 15 of tile t).  Blocks at or past b_hi and chunks at or past K read a clamped (valid)
// address; their products are masked on the activation side.
template <int NT, int PRE>
__device__ __forceinline__ void load_w(const bf16_t* const (&wrow)[NT], int blk, int b_hi, int K, WFrag<NT, PRE>& f) {
  const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int k = (blk + it) * 64 + g * 16 + s * 8;
      const int kk = (blk + it < b_hi && k < K) ? k : 0;
#pragma unroll
      for (int t = 0; t < NT; ++t) f.a[it][t][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow[t] + kk));
    }
  }
}

// ---------------------------------------------------------------- norm prologue, one wave per row
template <int XC>
struct RowW {
  u32x4_t v[XC][4];                   // chunk (i, w): elements (i * 256 + w * 64 + lane) * 8 .. + 8, thread w * 64 + lane of stage_x
};
template <int XC>
__device__ __forceinline__ void load_row_w(const bf16_t* __restrict__ p, int K, RowW<XC>& r) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < XC; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = (i * 256 + w * 64 + lane) * 8;
      r.v[i][w] = *reinterpret_cast<const u32x4_t*>(p + (c < K ? c : 0));
    }
}
// xs[0..K) = stage_x's row, computed by ONE wave: for w = 0..3 it is wave w of stage_x (thread w * 64 + lane)
template <int XC>
__device__ __forceinline__ void norm_row_w(const RowW<XC>& xr, const RowW<XC>& gr, float eps, int K, bf16_t* xs) {
  const int lane = threadIdx.x & 63;
  float red[4];
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    const int tid = w * 64 + lane;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < XC; ++i) {
      float f[8];
      unpack8(xr.v[i][w], f);
      if ((i * 256 + tid) * 8 < K) {
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
      }
    }
    ss = wave_sum(ss);
    red[w] = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(ss)));       // stage_x keeps lane 0's total
  }
  const float r = rsqrtf((red[0] + red[1] + red[2] + red[3]) / (float)K + eps);
#pragma unroll
  for (int i = 0; i < XC; ++i)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int c = (i * 256 + w * 64 + lane) * 8;
      if (c < K) {
        float f[8], g[8];
        unpack8(xr.v[i][w], f);
        unpack8(gr.v[i][w], g);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = g[j] * rbf(f[j] * r);
        *reinterpret_cast<u32x4_t*>(xs + c) = pack8(f);
      }
    }
}

// ---------------------------------------------------------------- the fused core: norm prologue + 16 x B tile(s) over K
// 256 threads.  On return wave 0 holds in acc[t] the finished fp32 tile t: lane l has column (stream lane) l & 15, rows 4 (l >> 4) + reg.
template <int NT, int XC>
__device__ __forceinline__ void decw_fused_tiles(const svlm_lane* __restrict__ lanes, int B, const bf16_t* __restrict__ x, int ldx,
                                                 const bf16_t* __restrict__ ln_w, float eps, const bf16_t* const (&wrow)[NT], int K,
                                                 f32x4_t (&acc)[NT]) {
  constexpr int PRE = DECW_PRE;
  bf16_t* xs = reinterpret_cast<bf16_t*>(dyn_smem);
  __shared__ f32x4_t part[4][NT][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r = lane & 15, g = lane >> 4;
  const int ldxs = decw_ldxs_d(K);
  const int nblk = (K + 63) >> 6, bpw = (nblk + 3) >> 2;
  const int b_lo = wave * bpw, b_hi = min(nblk, b_lo + bpw);
  bool lv[4];                                                          // (wave-uniform) the rows this wave stages
#pragma unroll
  for (int q = 0; q < 4; ++q) lv[q] = wave + 4 * q < B && lane_live(lanes[min(wave + 4 * q, B - 1)]);
  RowW<XC> gr, xr[2];
  load_row_w<XC>(ln_w, K, gr);
  if (lv[0]) load_row_w<XC>(x + (size_t)wave * ldx, K, xr[0]);
  __builtin_amdgcn_sched_barrier(0);
  WFrag<NT, PRE> cur;
  load_w<NT, PRE>(wrow, b_lo, b_hi, K, cur);                          // the head of the weight stream is in flight during the norm
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (q < 3 && lv[q + 1]) load_row_w<XC>(x + (size_t)(wave + 4 * (q + 1)) * ldx, K, xr[(q + 1) & 1]);
    if (lv[q]) norm_row_w<XC>(xr[q & 1], gr, eps, K, xs + (size_t)(wave + 4 * q) * ldxs);
  }
  lds_barrier();
  const bf16_t* xsrow = xs + (size_t)min(r, B - 1) * ldxs;
  const bool colok = r < B;
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  for (int blk = b_lo; blk < b_hi; blk += PRE) {
    WFrag<NT, PRE> nxt;
    load_w<NT, PRE>(wrow, blk + PRE, b_hi, K, nxt);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k = (blk + it) * 64 + g * 16 + s * 8;
        const bool ok = colok && blk + it < b_hi && k < K;
        u32x4_t bv = *reinterpret_cast<const u32x4_t*>(xsrow + (k < K ? k : 0));
        if (!ok) bv = u32x4_t{0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(cur.a[it][t][s]), as_frag(bv), acc[t], 0, 0, 0);
      }
    }
    cur = nxt;
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) part[wave][t][lane] = acc[t];
  __syncthreads();
  if (wave == 0) {
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = part[0][t][lane] + part[1][t][lane] + part[2][t][lane] + part[3][t][lane];
  }
}

// ---------------------------------------------------------------- QKV + KV append
template <int XC>
__global__ __launch_bounds__(256) void decw_qkv_kernel(const svlm_lane* __restrict__ lanes, int B, const bf16_t* __restrict__ x, int ldx,
                                                       const bf16_t* __restrict__ ln_w, float eps, const bf16_t* __restrict__ W, int ldw,
                                                       const bf16_t* __restrict__ bias, bf16_t* __restrict__ q_out, int ldq, int layer,
                                                       int N, int K, int qd, int kd, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16;
  const bf16_t* wrow[1] = {W + (size_t)min(n0 + (lane & 15), N - 1) * ldw};
  f32x4_t acc[1];
  decw_fused_tiles<1, XC>(lanes, B, x, ldx, ln_w, eps, wrow, K, acc);
  if (wave != 0) return;
  const int b = lane & 15;
  if (b >= B || !lane_live(lanes[b])) return;
  const svlm_lane& L = lanes[b];
  const int Hkv = kd / D;
  const int row = L.state[0];
  const int slot = L.slot_of[row];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = n0 + 4 * (lane >> 4) + e;
    if (n >= N) break;
    const bf16_t v = f2bf(acc[0][e] + bf2f(bias[n]));
    if (n < qd) {
      q_out[(size_t)b * ldq + n] = v;
    } else {
      lane_kv_append(L, layer, Hkv, D, row, slot, n - qd, kd, v);
    }
  }
}

// ---------------------------------------------------------------- gate/up + SwiGLU
template <int XC>
__global__ __launch_bounds__(256) void decw_gate_up_kernel(const svlm_lane* __restrict__ lanes, int B, const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ ln_w, float eps, const bf16_t* __restrict__ W, int ldw,
                                                           bf16_t* __restrict__ h, int ldh, int I, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16;
  const int nr = min(n0 + (lane & 15), I - 1);
  const bf16_t* wrow[2] = {W + (size_t)nr * ldw, W + (size_t)(I + nr) * ldw};           // gate rows, up rows of the same outputs
  f32x4_t acc[2];
  decw_fused_tiles<2, XC>(lanes, B, x, ldx, ln_w, eps, wrow, K, acc);
  if (wave != 0) return;
  const int b = lane & 15;
  if (b >= B || !lane_live(lanes[b])) return;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = n0 + 4 * (lane >> 4) + e;
    if (n >= I) break;
    const float gv = rbf(acc[0][e]), uv = rbf(acc[1][e]);
    h[(size_t)b * ldh + n] = f2bf(apply_act(gv, SVLM_ACT_SILU) * uv);
  }
}

// ---------------------------------------------------------------- lm_head + penalty + argmax candidates
// A tile is two candidate groups of 8 vocabulary rows: rows 0..7 are held by lane groups 0 and 1, rows 8..15 by groups 2 and 3.
template <int XC>
__global__ __launch_bounds__(256) void decw_lm_head_kernel(const svlm_lane* __restrict__ lanes, int B, const bf16_t* __restrict__ x, int ldx,
                                                           const bf16_t* __restrict__ ln_w, float eps, const bf16_t* __restrict__ W, int ldw,
                                                           float* __restrict__ logits, int ldl, const int* __restrict__ suppress,
                                                           float* __restrict__ ws, long long ws_stride, int n_parts, int V, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n0 = blockIdx.x * 16;
  const bf16_t* wrow[1] = {W + (size_t)min(n0 + (lane & 15), V - 1) * ldw};
  f32x4_t acc[1];
  decw_fused_tiles<1, XC>(lanes, B, x, ldx, ln_w, eps, wrow, K, acc);
  if (wave != 0) return;
  const int b = lane & 15, g = lane >> 4;
  const bool live = b < B && lane_live(lanes[min(b, B - 1)]);
  float best = -INFINITY;
  int bi = 0x7fffffff;
  if (live) {
    const svlm_lane& L = lanes[b];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int n = n0 + 4 * g + e;
      if (n >= V) break;
      float v = rbf(acc[0][e]);
      logits[(size_t)b * ldl + n] = v;
      v = cand_score(v, n, L.seen, L.penalty, suppress, L.n_suppress, nullptr, 1.0f, L.state);
      cand_take(best, bi, v, n);
    }
  }
  const float ob = __shfl_down(best, 16, 64);            // the other half of the candidate group (rows 4 higher)
  const int oi = __shfl_down(bi, 16, 64);
  cand_take(best, bi, ob, oi);
  const int part = blockIdx.x * 2 + (g >> 1);
  if (live && (g & 1) == 0 && part < n_parts) {
    float* pv = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + (size_t)b * ws_stride);
    int* pi = reinterpret_cast<int*>(pv + n_parts);
    pv[part] = best;
    pi[part] = bi;
  }
}

// ---------------------------------------------------------------- residual GEMVs (o_proj, down_proj)
// y[b][n] = bf16(bf16(W[n] . x[b]) + residual[b][n]); `y` may be `residual`.  KW waves split K; the activations come from global
// memory (L2-resident) with the weights.
template <int PRE>
struct GFrag {
  u32x4_t a[PRE][2], b[PRE][2];
};
template <int PRE>
__device__ __forceinline__ void load_wx(const bf16_t* wrow, const bf16_t* xrow, int blk, int b_hi, int K, GFrag<PRE>& f) {
  const int g = (threadIdx.x & 63) >> 4;
#pragma unroll
  for (int it = 0; it < PRE; ++it) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int k = (blk + it) * 64 + g * 16 + s * 8;
      const int kk = (blk + it < b_hi && k < K) ? k : 0;
      f.a[it][s] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow + kk));
      f.b[it][s] = *reinterpret_cast<const u32x4_t*>(xrow + kk);
    }
  }
}

template <int KW>
__global__ __launch_bounds__(KW * 64) void decw_gemv_kernel(const svlm_lane* __restrict__ lanes, int B, const bf16_t* __restrict__ x, int ldx,
                                                            const bf16_t* __restrict__ W, int ldw, const bf16_t* residual, int ldr,
                                                            bf16_t* y, int ldy, int N, int K) {
  constexpr int PRE = DECW_PRE_GEMV;
  __shared__ f32x4_t part[KW][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const bf16_t* wrow = W + (size_t)min(n0 + r, N - 1) * ldw;
  const bf16_t* xrow = x + (size_t)min(r, B - 1) * ldx;
  const bool colok = r < B;
  const int nblk = (K + 63) >> 6, bpw = (nblk + KW - 1) / KW;
  const int b_lo = wave * bpw, b_hi = min(nblk, b_lo + bpw);
  f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
  GFrag<PRE> cur;
  load_wx<PRE>(wrow, xrow, b_lo, b_hi, K, cur);
  for (int blk = b_lo; blk < b_hi; blk += PRE) {
    GFrag<PRE> nxt;
    load_wx<PRE>(wrow, xrow, blk + PRE, b_hi, K, nxt);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int it = 0; it < PRE; ++it) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int k = (blk + it) * 64 + g * 16 + s * 8;
        u32x4_t bv = cur.b[it][s];
        if (!(colok && blk + it < b_hi && k < K)) bv = u32x4_t{0u, 0u, 0u, 0u};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(cur.a[it][s]), as_frag(bv), acc, 0, 0, 0);
      }
    }
    cur = nxt;
  }
  part[wave][lane] = acc;
  __syncthreads();
  if (wave != 0) return;
  if (!colok || !lane_live(lanes[r])) return;
  f32x4_t sum = part[0][lane];
#pragma unroll
  for (int w = 1; w < KW; ++w) sum += part[w][lane];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int n = n0 + 4 * g + e;
    if (n >= N) break;
    y[(size_t)r * ldy + n] = resid_tail(sum[e], residual[(size_t)r * ldr + n]);
  }
}

// ================================================================ launchers
static inline int decw_gemv_kw(int K) {
  const int nblk = (K + 63) / 64;
  return nblk >= 64 ? 16 : (nblk >= 16 ? 8 : 4);
}

extern "C" int svlm_decw_max_lanes(void) { return DECW_MAX_LANES; }

extern "C" int svlm_decw_plan(int fused, int K, int* splits, int* kps) {
  if (K <= 0 || K % 8 != 0 || splits == nullptr || kps == nullptr) return SVLM_EINVAL;
  const int kw = fused ? 4 : decw_gemv_kw(K);
  const int nblk = (K + 63) / 64;
  *splits = kw;
  *kps = (nblk + kw - 1) / kw * 64;
  return SVLM_OK;
}

static inline bool decw_lanes_ok(const void* lanes, int B) { return lanes != nullptr && B >= 1 && B <= DECW_MAX_LANES; }
static inline bool decw_fused_ok(int B, int K, int ldx) {
  return K > 0 && K % 8 == 0 && K <= 4096 && (long long)B * decw_ldxs(K) * 2 <= DECW_LDS_DYN_MAX && ldx >= K && ldx % 8 == 0;
}

// the staged rows of many lanes pass the 64 KB of dynamic LDS a launch gets without opting in
extern "C" int svlm_decw_reserve_lds(void) {
  static bool done = false;
  if (done) return SVLM_OK;
  const void* k[6] = {reinterpret_cast<const void*>(&decw_qkv_kernel<1>),     reinterpret_cast<const void*>(&decw_qkv_kernel<2>),
                      reinterpret_cast<const void*>(&decw_gate_up_kernel<1>), reinterpret_cast<const void*>(&decw_gate_up_kernel<2>),
                      reinterpret_cast<const void*>(&decw_lm_head_kernel<1>), reinterpret_cast<const void*>(&decw_lm_head_kernel<2>)};
  for (int i = 0; i < 6; ++i) {
    hipError_t e = hipFuncSetAttribute(k[i], hipFuncAttributeMaxDynamicSharedMemorySize, DECW_LDS_DYN_MAX);
    if (e != hipSuccess) {
      svlm_set_error("svlm_decw_reserve_lds: cannot reserve %d B of LDS: %s", DECW_LDS_DYN_MAX, hipGetErrorString(e));
      return SVLM_ELAUNCH;
    }
  }
  done = true;
  return SVLM_OK;
}

#define DECW_XC(KERNEL, K, ...)                          \
  do {                                                   \
    if ((K) <= 2048) KERNEL<1> __VA_ARGS__;              \
    else KERNEL<2> __VA_ARGS__;                          \
  } while (0)

extern "C" int svlm_decw_embed(const void* lanes, int B, const void* table, int n_rows, void* x, int ldx, int cols, void* stream) {
  SVLM_CHECK_ARG(decw_lanes_ok(lanes, B) && n_rows > 0 && cols > 0 && cols % 8 == 0 && ldx >= cols && ldx % 8 == 0,
                 "svlm_decw_embed: bad B=%d n_rows=%d cols=%d ldx=%d", B, n_rows, cols, ldx);
  decb_embed_launch(lanes, B, table, n_rows, x, ldx, cols, stream);
  return svlm_check_launch("svlm_decw_embed");
}

extern "C" int svlm_decw_qkv(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W, int ldw,
                             const void* bias, void* q_out, int ldq, int layer, int K, int qd, int kd, int D, void* stream) {
  SVLM_CHECK_ARG(decw_lanes_ok(lanes, B) && decw_fused_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0,
                 "svlm_decw_qkv: bad B=%d K=%d ldx=%d ldw=%d (1..16 lanes, K a multiple of 8 up to 4096, the staged rows within %d B of LDS)", B, K,
                 ldx, ldw, DECW_LDS_DYN_MAX);
  if (!decb_qkv_args_ok("svlm_decw_qkv", qd, kd, D, bias, ldq, layer)) return SVLM_EINVAL;
  const int N = qd + 2 * kd, dyn = B * decw_ldxs(K) * 2;
  if (dyn > 65536 && svlm_decw_reserve_lds() != SVLM_OK) return SVLM_ELAUNCH;
  DECW_XC(decw_qkv_kernel, K, <<<(N + 15) / 16, 256, dyn, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, B, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, (const bf16_t*)bias, (bf16_t*)q_out,
      ldq, layer, N, K, qd, kd, D));
  return svlm_check_launch("svlm_decw_qkv");
}

extern "C" int svlm_decw_gate_up(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W, int ldw,
                                 void* h, int ldh, int I, int K, void* stream) {
  SVLM_CHECK_ARG(decw_lanes_ok(lanes, B) && decw_fused_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0 && I > 0 && ldh >= I,
                 "svlm_decw_gate_up: bad B=%d I=%d K=%d ldx=%d ldw=%d ldh=%d (1..16 lanes, K a multiple of 8 up to 4096, the staged rows within %d B "
                 "of LDS)", B, I, K, ldx, ldw, ldh, DECW_LDS_DYN_MAX);
  const int dyn = B * decw_ldxs(K) * 2;
  if (dyn > 65536 && svlm_decw_reserve_lds() != SVLM_OK) return SVLM_ELAUNCH;
  DECW_XC(decw_gate_up_kernel, K, <<<(I + 15) / 16, 256, dyn, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, B, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, (bf16_t*)h, ldh, I, K));
  return svlm_check_launch("svlm_decw_gate_up");
}

extern "C" int svlm_decw_gemv(const void* lanes, int B, const void* x, int ldx, const void* W, int ldw, const void* residual, int ldr,
                              void* y, int ldy, int N, int K, void* stream) {
  SVLM_CHECK_ARG(decw_lanes_ok(lanes, B) && N > 0 && K > 0 && K % 8 == 0 && ldw % 8 == 0 && ldw >= K && ldx >= K && ldx % 8 == 0,
                 "svlm_decw_gemv: bad shape B=%d N=%d K=%d ldw=%d ldx=%d (1..16 lanes, K a multiple of 8)", B, N, K, ldw, ldx);
  SVLM_CHECK_ARG(residual != nullptr && y != nullptr && ldr >= N && ldy >= N, "svlm_decw_gemv: residual and y are required (ldr=%d ldy=%d)", ldr, ldy);
  hipStream_t s = (hipStream_t)stream;
  const int kw = decw_gemv_kw(K), tiles = (N + 15) / 16;
#define DECW_GEMV_ARGS (const svlm_lane*)lanes, B, (const bf16_t*)x, ldx, (const bf16_t*)W, ldw, (const bf16_t*)residual, ldr, (bf16_t*)y, ldy, N, K
  if (kw == 16) decw_gemv_kernel<16><<<tiles, 1024, 0, s>>>(DECW_GEMV_ARGS);
  else if (kw == 8) decw_gemv_kernel<8><<<tiles, 512, 0, s>>>(DECW_GEMV_ARGS);
  else decw_gemv_kernel<4><<<tiles, 256, 0, s>>>(DECW_GEMV_ARGS);
#undef DECW_GEMV_ARGS
  return svlm_check_launch("svlm_decw_gemv");
}

extern "C" int svlm_decw_lm_head(const void* lanes, int B, const void* x, int ldx, const void* ln_w, float eps, const void* W, int ldw,
                                 float* logits, int ldl, const int* suppress, void* ws, int V, int K, void* stream) {
  SVLM_CHECK_ARG(decw_lanes_ok(lanes, B) && decw_fused_ok(B, K, ldx) && ldw >= K && ldw % 8 == 0 && V > 0 && ldl >= V,
                 "svlm_decw_lm_head: bad B=%d V=%d K=%d ldx=%d ldw=%d ldl=%d (1..16 lanes, K a multiple of 8 up to 4096, the staged rows within %d B "
                 "of LDS)", B, V, K, ldx, ldw, ldl, DECW_LDS_DYN_MAX);
  SVLM_CHECK_ARG(ws != nullptr && logits != nullptr, "svlm_decw_lm_head: null logits / workspace");
  const int dyn = B * decw_ldxs(K) * 2;
  if (dyn > 65536 && svlm_decw_reserve_lds() != SVLM_OK) return SVLM_ELAUNCH;
  const int n_parts = (V + 7) / 8;                 // = the candidate count of svlm_decb_lm_head, whose finish kernel reads them
  DECW_XC(decw_lm_head_kernel, K, <<<(V + 15) / 16, 256, dyn, (hipStream_t)stream>>>(
      (const svlm_lane*)lanes, B, (const bf16_t*)x, ldx, (const bf16_t*)ln_w, eps, (const bf16_t*)W, ldw, logits, ldl, suppress, (float*)ws,
      svlm_decb_lm_head_ws_stride(V), n_parts, V, K));
  return svlm_check_launch("svlm_decw_lm_head");
}

extern "C" int svlm_decw_argmax_finish(const void* lanes, int B, const void* ws, int V, int advance_kv, void* stream) {
  SVLM_CHECK_ARG(decw_lanes_ok(lanes, B) && V > 0 && ws != nullptr, "svlm_decw_argmax_finish: bad args (B=%d V=%d)", B, V);
  decb_argmax_finish_launch(lanes, B, ws, V, advance_kv, stream);
  return svlm_check_launch("svlm_decw_argmax_finish");
}
