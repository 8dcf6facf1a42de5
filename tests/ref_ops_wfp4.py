"""TEST-ONLY CPU reference of the weight-fp4 prefill GEMMs (csrc/gemm_wfp4.hip): `gemm` / `gemm_norm` of the bf16 reference on
W' = dequantize_blocks_mxfp4(W4, w_scale) -- the operands the kernel's MFMAs are fed, so what it computes up to the fp32 summation
order."""
from __future__ import annotations

from ref_ops_fp4 import RefOpsFp4

from streaming_vlm_amd.weights import dequantize_blocks_mxfp4


class RefOpsWfp4(RefOpsFp4):
    name = "ref-cpu-wfp4"

    def gemm_wfp4(self, A, W4, w_scale, bias=None, residual=None, out=None, act=0):
        return self.gemm(A, dequantize_blocks_mxfp4(W4, w_scale), bias=bias, residual=residual, out=out, act=act)

    def gemm_wfp4_norm(self, A, W4, w_scale, norm_w, eps, out, out_norm, bias=None, residual=None, act=0, norm_b=None):
        return self.gemm_norm(A, dequantize_blocks_mxfp4(W4, w_scale), norm_w, eps, out, out_norm, bias=bias, residual=residual, act=act,
                              norm_b=norm_b)
