// What the lane-batched decode kernels share whatever their weights: the lane table and its side tables, the activation-row prologue,
// and a lane's KV append.  Included by decode_batch.hip (bf16), decode_batch_fp8.hip (e4m3),
// decode_batch_fp4.hip (MXFP4), decode_wide.hip (MFMA, bf16) and decode_attn.hip (svlm_decb_attn); the kernel shells of the first three
// are in dec_shell.h.
#pragma once
#include "common.h"
#include "dec_xrow.h"
#include "dec_epi.h"

struct svlm_lane {                 // mirror of include/svlm.h
  bf16_t* pool;                    // [n_layers][2][Hkv][n_slots][D]
  bf16_t* lin;                     // [n_layers][2][Hkv][lin_rows][D] or null
  const int* slot_of;
  int* state;                      // {kv_len, cur}
  int* tok_buf;
  unsigned char* seen;             // [V] or null (no repetition penalty)
  int limit;                       // live while state[1] + 1 < limit
  int n_slots;
  int lin_rows;
  float penalty;
  int n_suppress;
  int pad_;
};
static_assert(sizeof(svlm_lane) == 72, "svlm_lane layout (include/svlm.h)");

// The sampling record of a lane, in a table of its own parallel to the lane table (svlm_decb_lm_head_sample / svlm_decb_sample_finish).
struct svlm_lane_sample {          // mirror of include/svlm.h
  const unsigned* rng;             // {seed lo, seed hi} of the lane's current generate() call, or null (greedy)
  float inv_temp;                  // fp32(1) / fp32(temperature), divided on the host as the single-row entries do
  int top_k;
  float top_p;
  int mode;                        // SVLM_SAMPLE_*
};
static_assert(sizeof(svlm_lane_sample) == 24, "svlm_lane_sample layout (include/svlm.h)");
enum { SVLM_SAMPLE_GREEDY = 0, SVLM_SAMPLE_GUMBEL = 1, SVLM_SAMPLE_FILTERED = 2, SVLM_SAMPLE_NUCLEUS = 3 };

// The attention record of a lane, in a table of its own parallel to the lane table (svlm_decb_attn, decode_attn.hip): what the
// single-stream decode attention takes as arguments and the lane record does not hold.
struct svlm_lane_attn {            // mirror of include/svlm.h
  const bf16_t* rope_cs;           // the lane's cos / sin table [>= attn_len][D]
  const int* lin_len_dev;          // lin_state {rows rotated, fresh rows follow} of the lane's linear planes, or null (no planes)
  float* ws;                       // the lane's decode workspace, svlm_decode_attn_ws_bytes(Hq, attn_len, chunk)
  int attn_len;                    // max_len of the single-lane call: the split count is ceil(attn_len / chunk)
  int chunk;                       // keys per workgroup
};
static_assert(sizeof(svlm_lane_attn) == 32, "svlm_lane_attn layout (include/svlm.h)");

// host side, defined in decode_batch.hip: the candidate workspace stride, and the launches of the embed and finish kernels without the
// B <= 4 check of their entries (shared with the wide entries of decode_wide.hip)
extern "C" long long svlm_decb_lm_head_ws_stride(int V);
void decb_embed_launch(const void* lanes, int B, const void* table, int n_rows, void* x, int ldx, int cols, void* stream);
void decb_argmax_finish_launch(const void* lanes, int B, const void* ws, int V, int advance_kv, void* stream);

__device__ __forceinline__ bool lane_live(const svlm_lane& L) { return L.state[1] + 1 < L.limit; }

// kv_append (dec_epi.h) for a lane: column j of the [k | v] output of the lane's new token at logical row `row`, into the planes of
// `layer` in the lane's own pool and, if it has them, linear planes.  Only the base of the plane column j belongs to is computed (it
// stands for both of kv_append's bases).
__device__ __forceinline__ void lane_kv_append(const svlm_lane& L, int layer, int Hkv, int D, int row, int slot, int j, int kd, bf16_t v) {
  const int p = layer * 2 + (j < kd ? 0 : 1);
  bf16_t* plane = L.pool + (size_t)p * Hkv * L.n_slots * D;
  bf16_t* lp = L.lin != nullptr ? L.lin + (size_t)p * Hkv * L.lin_rows * D : nullptr;
  kv_append(plane, plane, L.n_slots, lp, lp, L.lin_rows, row, slot, j, kd, D, v);
}

// Prologue of the fused kernels: the live lanes' x rows are requested first, then the head of the weight stream, then the rows are
// normalised and staged one after the other (xs[b * K ..]); a lane that is not live leaves its LDS row as it is (its products are
// never written).
template <int NB, int XC>
__device__ __forceinline__ void load_rows(const svlm_lane* __restrict__ lanes, const bf16_t* __restrict__ x, int ldx,
                                          const bf16_t* __restrict__ ln_w, int K, XRow<XC> (&xr)[NB], bool (&live)[NB]) {
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    live[b] = lane_live(lanes[b]);
    if (live[b]) load_x<XC>(x + (size_t)b * ldx, ln_w, K, xr[b]);
  }
}
template <int NB, int XC>
__device__ __forceinline__ void stage_rows(const XRow<XC> (&xr)[NB], const bool (&live)[NB], float eps, int K, bf16_t* xs) {
#pragma unroll
  for (int b = 0; b < NB; ++b)
    if (live[b]) stage_x<XC>(xr[b], eps, K, xs + (size_t)b * K);          // (workgroup-uniform branch: barriers inside)
}
