"""ctypes binding of libsvlm_hip.so (C ABI declared in include/svlm.h).

The product path has NO fallback: if the shared library is missing or a call fails, this module
raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"`` (hipcc, gfx950).
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SVLM_LIB_PATH") or os.path.join(_HERE, "libsvlm_hip.so")      # override: diagnostic builds (tools/)

SVLM_OK = 0
ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF, ACT_SILU, ACT_SWIGLU = 0, 1, 2, 3, 4


class SvlmError(RuntimeError):
    pass


_p, _i, _f, _ll = C.c_void_p, C.c_int, C.c_float, C.c_longlong

# name -> (restype, argtypes); must list every symbol of include/svlm.h (tests/test_abi.py checks it)
SIGNATURES = {
    "svlm_abi_version": (_i, []),
    "svlm_last_error": (C.c_char_p, []),
    "svlm_device_cus": (_i, []),
    "svlm_gemm_bf16": (_i, [_p, _i, _p, _i, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p]),
    "svlm_gemm_bf16_norm": (_i, [_p, _i, _p, _i, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _f, _p, _i, _p]),
    "svlm_quant_rows_fp8": (_i, [_p, _i, _p, _i, _p, _i, _i, _p]),
    "svlm_gemm_fp8": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _f, _p, _i, _p]),
    "svlm_gemm_fp8_normq": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _f, _p, _i, _p, _i, _p, _p]),
    "svlm_gemv_bf16": (_i, [_p, _p, _i, _p, _p, _p, _p, _i, _i, _i, _p]),
    "svlm_prefetch": (_i, [_p, _ll, _i, _p]),
    "svlm_rmsnorm": (_i, [_p, _p, _p, _i, _i, _f, _p]),
    "svlm_layernorm": (_i, [_p, _p, _p, _p, _i, _i, _f, _p]),
    "svlm_add": (_i, [_p, _p, _p, _ll, _p]),
    "svlm_silu_mul": (_i, [_p, _p, _i, _i, _p]),
    "svlm_gather_rows": (_i, [_p, _p, _p, _p, _p, _i, _i, _p]),
    "svlm_patchify_u8": (_i, [_p, _p, _i, _i, _i, _i, _i, _i, _f, _f, _f, _f, _f, _f, _p]),
    "svlm_resize_aa_tables": (_i, [_i, _i, _p, _p, _p, _i]),
    "svlm_resize_ws_bytes": (_ll, [_i, _i, _i]),
    "svlm_resize_bicubic_aa_u8": (_i, [_p, _p, _i, _i, _i, _i, _i, _p, _p, _p, _i, _p, _p, _p, _i, _p, _ll, _p]),
    "svlm_vit_rope": (_i, [_p, _p, _p, _i, _i, _i, _p]),
    "svlm_vit_attn": (_i, [_p, _p, _i, _i, _i, _i, _f, _p]),
    "svlm_mrope_table": (_i, [_p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "svlm_rope_index_ws_bytes": (_ll, [_i, _i]),
    "svlm_rope_index": (_i, [_p, _i, _p, _i, _i, _i, _i, _p, _p, _i, _f, _f, _i, _p, _ll, _p]),
    "svlm_evict_plan_ws_bytes": (_ll, [_i]),
    "svlm_evict_plan": (_i, [_p, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _p, _p, _ll, _p]),
    "svlm_kv_append": (_i, [_p, _i, _p, _i, _p, _p, _p, _p, _i, _i, _i, _i, _i, _p]),
    "svlm_kv_move_rows": (_i, [_p, _ll, _i, _i, _p, _p, _i, _p]),
    "svlm_kv_gather": (_i, [_p, _p, _p, _i, _i, _i, _i, _p]),
    "svlm_decode_attn_ws_bytes": (_ll, [_i, _i, _i]),
    "svlm_decode_attn_ropeload": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p]),
    "svlm_prefill_attn_ws_bytes": (_ll, [_i, _i, _i, _i]),
    "svlm_prefill_attn_ropeload": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _p, _ll, _p]),
    "svlm_prefill_attn_ropeload_lin": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _p, _ll, _p, _p, _i, _p, _p]),
    "svlm_decode_attn_lin": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _f, _p]),
    "svlm_mark_seen": (_i, [_p, _i, _p, _i, _p]),
    "svlm_argmax_ws_bytes": (_ll, []),
    "svlm_penalty_argmax": (_i, [_p, _i, _p, _f, _p, _i, _p, _p, _i, _p, _p]),
    "svlm_penalty_sample": (_i, [_p, _i, _p, _f, _p, _i, _f, _i, _f, _p, _p, _p, _i, _p, _p]),
    "svlm_dec_lm_head_sample": (_i, [_p, _p, _f, _p, _i, _p, _p, _f, _p, _i, _p, _i, _i, _f, _p, _p, _p]),
    "svlm_dec_qkv": (_i, [_p, _p, _f, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "svlm_dec_qkv_lin": (_i, [_p, _p, _f, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p]),
    "svlm_dec_gate_up": (_i, [_p, _p, _f, _p, _i, _p, _i, _i, _p]),
    "svlm_dec_tail_supported": (_i, [_i, _i, _i, _i, _i]),
    "svlm_dec_tail_ws_bytes": (_ll, [_i, _i, _i]),
    "svlm_dec_tail_reset": (_i, [_p, _i, _i, _i, _p]),
    "svlm_dec_tail": (_i, [_p, _p, _p, _i, _p, _p, _i, _p, _i, _p, _p, _i, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _i, _f, _p, _i, _i, _i, _p, _p]),
    "svlm_dec_lm_head_ws_bytes": (_ll, [_i]),
    "svlm_dec_lm_head": (_i, [_p, _p, _f, _p, _i, _p, _p, _f, _p, _i, _p, _i, _i, _p]),
    "svlm_argmax_finish": (_i, [_p, _i, _p, _p, _p, _i, _p]),
    "svlm_dec_qkv_fp8": (_i, [_p, _p, _f, _p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p]),
    "svlm_dec_gate_up_fp8": (_i, [_p, _p, _f, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_gemv_fp8": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "svlm_dec_lm_head_fp8": (_i, [_p, _p, _f, _p, _i, _p, _p, _p, _f, _p, _i, _p, _i, _i, _p]),
    "svlm_dec_lm_head_sample_fp8": (_i, [_p, _p, _f, _p, _i, _p, _p, _p, _f, _p, _i, _p, _i, _i, _f, _p, _p, _p]),
    "svlm_dequant_fp8_bf16": (_i, [_p, _p, _p, _i, _i, _p]),
    "svlm_gemm_wfp8": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p]),
    "svlm_gemm_wfp8_norm": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _f, _p, _i, _p]),
    "svlm_dec_qkv_fp4": (_i, [_p, _p, _f, _p, _i, _p, _p, _p, _p, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p, _p, _i, _p]),
    "svlm_dec_gate_up_fp4": (_i, [_p, _p, _f, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_gemv_fp4": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _i, _i, _i, _p]),
    "svlm_dequant_fp4_bf16": (_i, [_p, _p, _p, _i, _i, _p]),
    "svlm_gemm_wfp4": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p]),
    "svlm_gemm_wfp4_norm": (_i, [_p, _i, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _f, _p, _i, _p]),
    "svlm_quant_mxfp8": (_i, [_p, _i, _p, _i, _p, _i, _i, _p]),
    "svlm_gemm_mx_a8w4": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p]),
    "svlm_gemm_mx_a8w4_norm": (_i, [_p, _i, _p, _p, _i, _p, _p, _p, _i, _p, _i, _i, _i, _i, _i, _p, _ll, _p, _p, _f, _p, _i, _p]),
    "svlm_decb_embed": (_i, [_p, _i, _p, _i, _p, _i, _i, _p]),
    "svlm_decb_qkv": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "svlm_decb_gate_up": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _i, _i, _i, _p]),
    "svlm_decb_gemv": (_i, [_p, _i, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _p]),
    "svlm_decb_lm_head_ws_stride": (_ll, [_i]),
    "svlm_decb_lm_head": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_decb_argmax_finish": (_i, [_p, _i, _p, _i, _i, _p]),
    "svlm_decw_max_lanes": (_i, []),
    "svlm_decw_plan": (_i, [_i, _i, _p, _p]),
    "svlm_decw_reserve_lds": (_i, []),
    "svlm_decw_embed": (_i, [_p, _i, _p, _i, _p, _i, _i, _p]),
    "svlm_decw_qkv": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "svlm_decw_gate_up": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _i, _i, _i, _p]),
    "svlm_decw_gemv": (_i, [_p, _i, _p, _i, _p, _i, _p, _i, _p, _i, _i, _i, _p]),
    "svlm_decw_lm_head": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_decw_argmax_finish": (_i, [_p, _i, _p, _i, _i, _p]),
    "svlm_decb_qkv_fp8": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "svlm_decb_gate_up_fp8": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _i, _i, _i, _p]),
    "svlm_decb_gemv_fp8": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _i, _p, _i, _i, _i, _p]),
    "svlm_decb_lm_head_fp8": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_decb_qkv_fp4": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _p, _i, _i, _i, _i, _i, _i, _p]),
    "svlm_decb_gate_up_fp4": (_i, [_p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _i, _i, _i, _p]),
    "svlm_decb_gemv_fp4": (_i, [_p, _i, _p, _i, _p, _i, _p, _p, _i, _p, _i, _i, _i, _p]),
    "svlm_decb_lm_head_sample": (_i, [_p, _p, _i, _p, _i, _p, _f, _p, _i, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_decb_lm_head_sample_fp8": (_i, [_p, _p, _i, _p, _i, _p, _f, _p, _i, _p, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_decb_sample_finish": (_i, [_p, _p, _i, _p, _i, _p, _p, _i, _i, _p]),
    "svlm_decb_attn_max_lanes": (_i, []),
    "svlm_decb_attn": (_i, [_p, _p, _i, _p, _i, _p, _i, _i, _i, _i, _i, _f, _p, _p, _p, _p]),
}

_lib = None
_extra = {}          # explicit path -> handle (the diagnostic library next to the product one)

# exported by the diagnostic build (-DSVLM_TUNING) only; bound when present, never part of include/svlm.h
DIAG_SIGNATURES = {
    "svlm_diag_last_gemm_plan": (_i, [_p, _i]),
}
DIAG_LIB_PATH = os.path.join(_HERE, "build", "libsvlm_hip_diag.so")


def _bind(path):
    if not os.path.exists(path):
        raise SvlmError(
            f"{path} not found: the HIP extension is not built. Run `python -c \"import __graft_entry__ as g; "
            f"g.build()\"` at the repo root (needs hipcc). There is no fallback path.")
    lib = C.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError = ABI mismatch: fail loudly
        fn.restype = res
        fn.argtypes = args
    for name, (res, args) in DIAG_SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype = res
            fn.argtypes = args
    if lib.svlm_abi_version() != 1:
        raise SvlmError(f"{os.path.basename(path)} ABI version {lib.svlm_abi_version()} != 1")
    return lib


def load(path=None):
    """Load the library once; raise loudly when it is absent (no CPU / torch fallback exists).  `path`: another build of the same
    ABI (the diagnostic library), bound once per path next to the product handle."""
    global _lib
    if path is not None:
        key = os.path.abspath(path)
        if key not in _extra:
            _extra[key] = _bind(key)
        return _extra[key]
    if _lib is None:
        _lib = _bind(LIB_PATH)
    return _lib


def check(rc: int, what: str = "", lib=None):
    if rc != SVLM_OK:
        msg = (lib or load()).svlm_last_error()
        raise SvlmError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")
