"""TEST-ONLY CPU reference of the weight-fp8 prefill GEMMs (csrc/gemm_wfp8.hip): `gemm` / `gemm_norm` of the bf16 reference on
W' = dequantize_rows_fp8(W8, w_scale) -- the operands the kernel's MFMAs are fed, so what it computes up to the fp32 summation order."""
from __future__ import annotations

from ref_ops_fp8 import RefOpsFp8

from streaming_vlm_amd.weights import dequantize_rows_fp8


class RefOpsWfp8(RefOpsFp8):
    name = "ref-cpu-wfp8"

    def gemm_wfp8(self, A, W8, w_scale, bias=None, residual=None, out=None, act=0):
        return self.gemm(A, dequantize_rows_fp8(W8, w_scale), bias=bias, residual=residual, out=out, act=act)

    def gemm_wfp8_norm(self, A, W8, w_scale, norm_w, eps, out, out_norm, bias=None, residual=None, act=0, norm_b=None):
        return self.gemm_norm(A, dequantize_rows_fp8(W8, w_scale), norm_w, eps, out, out_norm, bias=bias, residual=residual, act=act,
                              norm_b=norm_b)
