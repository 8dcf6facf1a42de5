"""TEST-ONLY CPU reference of the MXFP4 language-model entry points (csrc/decode_fp4.hip): dequantise the e2m1 codes with their block
scales (W' = code * 2^e, exact in bf16) and call the bf16 reference op on W' -- which is what the kernels compute, up to the fp32
summation order.  The lm_head of an fp4 engine is e4m3: those entries are RefOpsFp8's."""
from __future__ import annotations

from ref_ops_fp8 import RefOpsFp8

from streaming_vlm_amd.weights import dequantize_blocks_mxfp4


class RefOpsFp4(RefOpsFp8):
    name = "ref-cpu-fp4"

    def dec_qkv_fp4(self, x, ln_w, eps, W4, w_scale, bias, q_out, pool, layer, slot_of, qd, kd, length=0, len_dev=None, lin=None):
        self.dec_qkv(x, ln_w, eps, dequantize_blocks_mxfp4(W4, w_scale), bias, q_out, pool, layer, slot_of, qd, kd, length=length,
                     len_dev=len_dev, lin=lin)

    def dec_gate_up_fp4(self, x, ln_w, eps, W4, w_scale, h):
        self.dec_gate_up(x, ln_w, eps, dequantize_blocks_mxfp4(W4, w_scale), h)

    def gemv_fp4(self, x, W4, w_scale, bias=None, residual=None, out=None, out_f32=None):
        return self.gemv(x, dequantize_blocks_mxfp4(W4, w_scale), bias=bias, residual=residual, out=out, out_f32=out_f32)

    def dequant_fp4(self, W4, w_scale, out):
        out.copy_(dequantize_blocks_mxfp4(W4, w_scale))
        return out
