"""TEST-ONLY CPU reference of the MX prefill (csrc/gemm_mx.hip): `quant_mxfp8` is weights.py:quantize_blocks_mxfp8, the definition the
kernel is held to bit for bit; `gemm_mx_a8w4[_norm]` is `gemm[_norm]` of the bf16 reference on (A', W') = (dequantize_blocks_mxfp8(A8, s),
dequantize_blocks_mxfp4(W4, s)) -- the operands the scaled MFMA multiplies, so what the kernel computes up to the fp32 summation order.
`k_halves=True` sums every MX GEMM as two K halves in fp32 before the one rounding to bf16: another legal summation order, whose
distance from the default one is the reference's own re-tiling noise (the floor the GPU test measures the kernel against)."""
from __future__ import annotations

import torch

from ref_ops import _act
from ref_ops_wfp4 import RefOpsWfp4

from streaming_vlm_amd.weights import dequantize_blocks_mxfp4, dequantize_blocks_mxfp8, dequantize_rows_fp8, quantize_blocks_mxfp8


class RefOpsMx(RefOpsWfp4):
    name = "ref-cpu-mx"

    def __init__(self, k_halves: bool = False):
        super().__init__()
        self.k_halves = bool(k_halves)
        self._heads = {}

    # the e4m3 lm_head of an fp4 engine, dequantised ONCE per matrix instead of at every decode step (same values as RefOpsFp8's entries)
    def _head(self, W8, w_scale):
        key = (W8.data_ptr(), w_scale.data_ptr(), tuple(W8.shape))
        if key not in self._heads:
            self._heads[key] = (dequantize_rows_fp8(W8, w_scale), W8, w_scale)
        return self._heads[key][0]

    def gemv_fp8(self, x, W8, w_scale, bias=None, residual=None, out=None, out_f32=None):
        return self.gemv(x, self._head(W8, w_scale), bias=bias, residual=residual, out=out, out_f32=out_f32)

    def dec_lm_head_fp8(self, x, ln_w, eps, W8, w_scale, logits, seen, penalty, suppress, ws, temperature=None, rng=None, state=None):
        self.dec_lm_head(x, ln_w, eps, self._head(W8, w_scale), logits, seen, penalty, suppress, ws, temperature=temperature, rng=rng, state=state)

    def quant_mxfp8(self, x, q=None, scale=None):
        codes, s = quantize_blocks_mxfp8(x)
        if q is not None:
            q.copy_(codes)
            codes = q
        if scale is not None:
            scale.copy_(s)
            s = scale
        return codes, s

    def _halves(self, A, W, bias, residual, out, act):
        h = A.shape[1] // 2 // 32 * 32
        Af, Wf = A.float(), W.float()
        y = Af[:, :h] @ Wf[:, :h].t()
        y = y + Af[:, h:] @ Wf[:, h:].t()
        if bias is not None:
            y = y + bias.float()
        y = y.to(torch.bfloat16)
        if act == 4:          # ACT_SWIGLU: W = [gate; up]
            I = y.shape[1] // 2
            y = torch.nn.functional.silu(y[:, :I]) * y[:, I:]
        else:
            y = _act(y, act)
            if residual is not None:
                y = residual + y
        if out is None:
            return y
        out.copy_(y)
        return out

    def gemm_mx_a8w4(self, A8, a_scale, W4, w_scale, bias=None, residual=None, out=None, act=0):
        A, W = dequantize_blocks_mxfp8(A8, a_scale), dequantize_blocks_mxfp4(W4, w_scale)
        if self.k_halves:
            return self._halves(A, W, bias, residual, out, act)
        return self.gemm(A, W, bias=bias, residual=residual, out=out, act=act)

    def gemm_mx_a8w4_norm(self, A8, a_scale, W4, w_scale, norm_w, eps, out, out_norm, bias=None, residual=None, act=0, norm_b=None):
        A, W = dequantize_blocks_mxfp8(A8, a_scale), dequantize_blocks_mxfp4(W4, w_scale)
        if not self.k_halves:
            return self.gemm_norm(A, W, norm_w, eps, out, out_norm, bias=bias, residual=residual, act=act, norm_b=norm_b)
        self._halves(A, W, bias, residual, out, act)
        if norm_b is None:
            self.rmsnorm(out, norm_w, eps, out=out_norm)
        else:
            self.layernorm(out, norm_w, norm_b, eps, out=out_norm)
        return out, out_norm
