// Host side of the decode launchers (decode_fused / _fp8 / _fp4, decode_batch / _fp8 / _fp4, decode_wide .hip): the lane-count switch
// and the qkv argument checks, once.
#pragma once
#include "common.h"

// The lane-count switch: the statement with NB, a compile-time constant, standing for B in 1..4 (the entries check the range).  Where
// a format takes another PRE at 3 and 4 lanes, the call site says so in terms of NB.
#define DECB_SWITCH_NB(B, ...)                                \
  do {                                                        \
    if ((B) == 1) { constexpr int NB = 1; __VA_ARGS__; }      \
    else if ((B) == 2) { constexpr int NB = 2; __VA_ARGS__; } \
    else if ((B) == 3) { constexpr int NB = 3; __VA_ARGS__; } \
    else { constexpr int NB = 4; __VA_ARGS__; }               \
  } while (0)

// The qkv arguments of a single-row entry `name` (`lin_name`: the name its linear-plane message carries): false, with the error text
// set, when the linear planes or the head geometry are not what the kernel takes.
static inline bool dec_qkv_args_ok(const char* name, const char* lin_name, int qd, int kd, int D, int n_slots, const void* bias,
                                   const void* k_lin, const void* v_lin, int lin_rows, const int* len_dev, int len_host) {
  if (!((k_lin == nullptr) == (v_lin == nullptr) &&
        (k_lin == nullptr || (D == 128 && lin_rows > 0 && lin_rows % 16 == 0 && (len_dev != nullptr || len_host < lin_rows))))) {
    svlm_set_error("%s: k_lin / v_lin come together, head_dim 128, lin_rows=%d a multiple of 16 above the row", lin_name, lin_rows);
    return false;
  }
  if (!(qd > 0 && kd > 0 && D > 0 && kd % D == 0 && n_slots > 0 && bias != nullptr)) {
    svlm_set_error("%s: bad qd=%d kd=%d D=%d", name, qd, kd, D);
    return false;
  }
  return true;
}
// ... of a lane-batched or wide entry
static inline bool decb_qkv_args_ok(const char* name, int qd, int kd, int D, const void* bias, int ldq, int layer) {
  if (qd > 0 && kd > 0 && D == 128 && kd % D == 0 && bias != nullptr && ldq >= qd && layer >= 0) return true;
  svlm_set_error("%s: bad qd=%d kd=%d D=%d ldq=%d layer=%d (head_dim 128)", name, qd, kd, D, ldq, layer);
  return false;
}
