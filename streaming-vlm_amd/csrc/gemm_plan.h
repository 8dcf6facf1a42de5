// Host pieces the prefill GEMM entries share (gemm.hip, gemm_fp8.hip, gemm_wfp8.hip, gemm_wfp4.hip, gemm_mx.hip): the cost model, the
// large-M rule, the split rounding, the grid size, the planner of the weight-code GEMMs and the launch helper.  The mirrors in
// tests/gemm_paths.py (_cost_plan, _large_m_bm, _finish_split, plan_wcode) are pinned to these by the no-GPU plan tests.
#pragma once
#include "common.h"
#include <stdio.h>
#include <stdlib.h>

// Tail shared by all GEMM entries (gemm.hip): split-K reduce (+ epilogue), with the norm of the output row folded in when there is
// one.  The partial slabs are plain fp32 (the fp8 kernel writes SCALED partials), so the bf16 reduce epilogues apply as they are.
int svlm_gemm_reduce_launch(const float* partial, int splits, const void* bias, const void* residual, int ldr, void* C, int ldc, int M, int N,
                            int act, const void* norm_w, const void* norm_b, float eps, void* XN, int ldxn, void* stream, void* XN8 = nullptr,
                            int ldxn8 = 0, float* xn_scale = nullptr);

// ---- tile height and K-split from a small cost model.  The path's GEMMs are one or two "rounds" of resident
// workgroups, so quantisation decides: cost = rounds x K-steps of 64 per workgroup x step cost (+ slab traffic).
// Resident workgroups per CU, bf16 tiles: LDS 2 x (BM+128) x 128 B -> 48 KB (BM=64): 3, 64 KB (BM=128): 2.  The weight-code GEMMs
// keep that residency in the model although their stages are smaller: a shape without a table entry then gets the K per split its
// bf16 twin gets and reproduces it bit for bit.
static inline void gemm_cost_plan(int M, int N, int K, int gn, const void* ws, long long ws_bytes, int* bm, int* splits) {
  int best_bm = 64, best_splits = 1;
  double best_cost = 1e30;
  for (int bm_c = 64; bm_c <= 128; bm_c += 64) {
    if (bm_c == 128 && M <= 64) continue;
    const long long tiles_c = (long long)((M + bm_c - 1) / bm_c) * gn;
    const long long cap = 256LL * (bm_c == 64 ? 3 : 2);
    const int max_s = ws != nullptr ? (K >= 1024 ? (K / 512 < 16 ? K / 512 : 16) : 1) : 1;
    for (int sp = 1; sp <= max_s; ++sp) {
      if (sp > 1 && (long long)sp * M * N * 4 > ws_bytes) break;
      const long long wgs = tiles_c * sp;
      const double rounds = (double)((wgs + cap - 1) / cap);
      const double ksteps = (double)((K + sp - 1) / sp + 64 - 1) / 64 + 3.0;                      // + prologue/epilogue
      const double step_us = bm_c == 64 ? 0.9 : 1.5;                                              // measured per K-step
      const double slab_us = sp > 1 ? 2.0 * sp * M * N * 4.0 / 3e12 * 1e6 + 5.0 : 0.0;            // slab write+read + reduce launch
      const double cost = rounds * ksteps * step_us + slab_us;
      if (cost < best_cost) { best_cost = cost; best_bm = bm_c; best_splits = sp; }
    }
  }
  *bm = best_bm;
  *splits = best_splits;
}

// Tile rows of an un-split large-M, long-K GEMM (M >= 2048, K >= 2048: the dense prefill's 4096-row passes): 256 x 128 tiles (8
// waves, one workgroup per CU) where their grid fills whole rounds of the 256 CUs, else 128-row tiles.  The measurements are with
// the rule's call in gemm.hip.
static inline int gemm_large_m_bm(int M, int gn) {
  const long long t256 = (long long)((M + 255) / 256) * gn;
  const long long rounds = (t256 + 255) / 256;
  return (t256 * 100 >= rounds * 256 * 85) ? 256 : 128;
}

// K per split as a multiple of the K-step `bk`, and the splits that are live with it
static inline void gemm_finish_split(int K, int bk, int* splits, int* kps) {
  *kps = K;
  if (*splits > 1) {
    *kps = ((K + *splits - 1) / *splits + bk - 1) / bk * bk;
    *splits = (K + *kps - 1) / *kps;
  }
}

// workgroups of a launch: one per (tile, split), or the un-split grid padded to the 8 XCDs (gemm_tile.h:gemm_tile_of)
static inline int gemm_grid_size(int gm, int gn, int splits) { return splits > 1 ? gn * gm * splits : 8 * ((gn + 7) / 8) * gm; }

// ---- the plan of the weight-code GEMMs (svlm_gemm_wfp8*, svlm_gemm_wfp4*): the cost model of svlm_gemm_bf16, the language-model
// shapes it mis-ranks, the large-M rule, the tuning switches `prefix`_NO_TABLE / _BM / _SPLITS, K-step 64.  Writes the plan note
// (`kind`: the note's fp8 field) before the caller makes its first device call.
struct GemmWPlan { int bm, gm, splits, kps, nblocks; };
static inline GemmWPlan gemm_wcode_plan(const char* prefix, int kind, int M, int N, int K, int gn, bool swiglu, const void* ws, long long ws_bytes) {
  auto env = [&](const char* suffix) {
    char name[48];
    snprintf(name, sizeof(name), "%s%s", prefix, suffix);
    return svlm_env(name);
  };
  GemmWPlan p;
  gemm_cost_plan(M, N, K, gn, ws, ws_bytes, &p.bm, &p.splits);
  // exact (N, K), row bucket ceil(M / 64) +- 1.  The split counts are those of the bf16 table (the prefill of a prefill_fp8 /
  // prefill_fp4 engine then equals the scratch-layer prefill bit for bit); these kernels have no tile taller than 128 rows below
  // M = 2048, so the 7B down_proj keeps its 8 splits on 128-row tiles.
  struct WfPlan { int mb, N, K, bm, splits; };
  static const WfPlan kPlans[] = {
      {5, 1536, 8960, 64, 4},      // Qwen2-VL-2B down_proj
      {5, 4608, 3584, 64, 2},      // 7B qkv
      {5, 3584, 3584, 64, 3},      // 7B o_proj
      {5, 3584, 18944, 128, 8},    // 7B down_proj
      {10, 3584, 18944, 128, 3},   // 7B down_proj at two temporal grids per chunk (M ~ 590)
      {10, 18944, 3584, 128, 1},   // 7B gate/up (SwiGLU pairing) at M ~ 590
      {5, 2560, 2048, 64, 3},      // Qwen2.5-VL-3B qkv
      {5, 2048, 2048, 64, 3},      // 3B o_proj
      {5, 2048, 11008, 64, 4},     // 3B down_proj
  };
  bool table_hit = false;
  if (env("_NO_TABLE") == nullptr) {
    const int mb = (M + 63) / 64;
    for (const WfPlan& t : kPlans) {
      if (t.N == N && t.K == K && mb >= t.mb - 1 && mb <= t.mb + 1 && (t.splits == 1 || (ws != nullptr && (long long)t.splits * M * N * 4 <= ws_bytes))) {
        p.bm = t.bm;
        p.splits = t.splits;
        table_hit = true;
        break;
      }
    }
  }
  if (M >= 2048 && K >= 2048 && p.splits == 1) p.bm = gemm_large_m_bm(M, gn);
  if (const char* force = env("_BM")) {       // tuning aid
    const int fb = atoi(force);
    p.bm = fb == 256 ? 256 : (fb == 128 ? 128 : 64);
    table_hit = false;
    if (const char* fs = env("_SPLITS")) p.splits = atoi(fs) > 0 ? atoi(fs) : 1; else p.splits = 1;
    if ((long long)p.splits * M * N * 4 > ws_bytes || ws == nullptr || K < 1024) p.splits = 1;
  }
  if (swiglu) p.splits = 1;        // one K pass: the pairing happens in the epilogue
  p.gm = (M + p.bm - 1) / p.bm;
  gemm_finish_split(K, 64, &p.splits, &p.kps);
  p.nblocks = gemm_grid_size(p.gm, gn, p.splits);
  SVLM_DIAG(g_svlm_gemm_plan_note = SvlmGemmPlanNote{g_svlm_gemm_plan_note.seq + 1, kind, p.bm, p.bm == 256 ? 8 : 4, 3, 1, p.splits, p.kps, table_hit ? 1 : 0, 0});
  return p;
}

// ---- launch of a tile kernel: reserves the dynamic LDS once per instantiation (on its first launch; the engine runs every shape
// eagerly before it captures a graph), launches, checks.  The arguments are cast to the kernel's parameter types.
template <auto KERNEL, int THREADS, int LDS, typename... P, typename... A>
static int gemm_launch_as(void (*)(P...), const char* entry, int nblocks, hipStream_t st, A... a) {
  static_assert(sizeof...(P) == sizeof...(A), "one argument per kernel parameter");
  static bool reserved = false;           // one flag per instantiation
  if (!reserved) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, LDS);
    if (e != hipSuccess) {
      svlm_set_error("%s: cannot reserve %d B of LDS: %s", entry, LDS, hipGetErrorString(e));
      return SVLM_ELAUNCH;
    }
    reserved = true;
  }
  KERNEL<<<dim3(nblocks, 1, 1), THREADS, LDS, st>>>((P)a...);
  return svlm_check_launch(entry);
}
template <auto KERNEL, int THREADS, int LDS, typename... A>
static int gemm_launch(const char* entry, int nblocks, hipStream_t st, A... a) {
  return gemm_launch_as<KERNEL, THREADS, LDS>(KERNEL, entry, nblocks, st, a...);
}
