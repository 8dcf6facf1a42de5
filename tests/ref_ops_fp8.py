"""TEST-ONLY CPU reference of the fp8 language-model entry points (csrc/decode_fp8.hip): dequantise the e4m3 rows with their
scales (W' = q * s, exact in bf16) and call the bf16 reference op on W' -- which is what the kernels compute, up to the fp32
summation order."""
from __future__ import annotations

from ref_ops import RefOps

from streaming_vlm_amd.weights import dequantize_rows_fp8


class RefOpsFp8(RefOps):
    name = "ref-cpu-fp8"

    def dec_qkv_fp8(self, x, ln_w, eps, W8, w_scale, bias, q_out, pool, layer, slot_of, qd, kd, length=0, len_dev=None, lin=None):
        self.dec_qkv(x, ln_w, eps, dequantize_rows_fp8(W8, w_scale), bias, q_out, pool, layer, slot_of, qd, kd, length=length,
                     len_dev=len_dev, lin=lin)

    def dec_gate_up_fp8(self, x, ln_w, eps, W8, w_scale, h):
        self.dec_gate_up(x, ln_w, eps, dequantize_rows_fp8(W8, w_scale), h)

    def gemv_fp8(self, x, W8, w_scale, bias=None, residual=None, out=None, out_f32=None):
        return self.gemv(x, dequantize_rows_fp8(W8, w_scale), bias=bias, residual=residual, out=out, out_f32=out_f32)

    def dec_lm_head_fp8(self, x, ln_w, eps, W8, w_scale, logits, seen, penalty, suppress, ws, temperature=None, rng=None, state=None):
        self.dec_lm_head(x, ln_w, eps, dequantize_rows_fp8(W8, w_scale), logits, seen, penalty, suppress, ws, temperature=temperature,
                         rng=rng, state=state)

    def dequant_fp8(self, W8, w_scale, out):
        out.copy_(dequantize_rows_fp8(W8, w_scale))
        return out
