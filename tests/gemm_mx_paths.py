"""Python mirror of the MX GEMM's dispatch (gemm_mx_impl in csrc/gemm_mx.hip), the operand builder and the case list of
tests/test_gemm_mx_gpu.py (test helper, not product; needs no GPU).  Operand generators: tests/gemm_paths.py and
tests/gemm_wfp4_paths.py."""
from __future__ import annotations

import torch

import gemm_paths as G
import gemm_wfp4_paths as P4

from streaming_vlm_amd.weights import (dequantize_blocks_mxfp4, dequantize_blocks_mxfp8, quantize_blocks_mxfp4,
                                       quantize_blocks_mxfp8)

BF16 = torch.bfloat16
WS_BYTES = G.WS_BYTES
KERNELS = {64: "mx<2>", 128: "mx<4>"}
_cdiv = G._cdiv
ref_columns = P4.ref_columns          # the 64 reference columns of a 7B-width case


def plan_mx(M, N, K, act=0, norm=False, env=None, ws_bytes=WS_BYTES):
    """-> dict(fp8=4, bm, waves, stages, dma, splits, kps, table, norm_fused, kernel).  N = output columns (SwiGLU: I)."""
    env = env or {}
    swiglu = act == 4
    gn = _cdiv(N, 64) if swiglu else _cdiv(N, 128)
    bm = 128 if M >= 1024 else 64
    splits = 1
    can_split = not swiglu
    tiles = _cdiv(M, bm) * gn
    if can_split and bm == 64 and tiles < 512 and K >= 1024:
        splits = min(_cdiv(512, tiles), K // 512, 8)
        while splits > 1 and splits * M * N * 4 > ws_bytes:
            splits -= 1
    if "SVLM_GEMM_MX_BM" in env and int(env["SVLM_GEMM_MX_BM"]) in (64, 128):
        bm = int(env["SVLM_GEMM_MX_BM"])
    if "SVLM_GEMM_MX_SPLITS" in env:
        v = int(env["SVLM_GEMM_MX_SPLITS"])
        if v == 1 or (1 < v <= K // 128 and can_split and v * M * N * 4 <= ws_bytes):
            splits = v
    if norm and splits == 1 and can_split and K >= 256 and 2 * M * N * 4 <= ws_bytes and N <= 4096:
        splits = 2
    splits, kps = G._finish_split(K, 128, splits)
    return dict(fp8=4, bm=bm, waves=4, stages=3, dma=1, splits=splits, kps=kps, table=0,
                norm_fused=int(bool(norm) and splits > 1 and N <= 4096), kernel=KERNELS[bm])


def operands(gen, M, N, K, bias=False, res=False, swiglu=False):
    """-> dict(A8 (M, K) uint8 e4m3 codes, sa (M, K / 32) uint8, Ap = A' (M, K) bf16, W4 (Nw, K / 2) uint8, s (Nw, K / 32) uint8,
    Wp = W' (Nw, K) bf16, bias, res) on the CPU: gemm_paths.operands with A quantised to MXFP8 and W to MXFP4; the reference multiplies
    A' by W'.
    blocks: gemm_wfp4_paths' `blocks` W (every (row, block) its own scale byte) and the one-hot A of `rowcol` with the 1 of row m
            replaced by 2^((7 m) % 11 - 5): the one non-zero block of an A row carries a scale byte of its own (114 .. 124, never the
            127 of the all-zero blocks around it), so an A scale taken from the wrong block, row, K-step or split offset shows as a
            wrong power of two at a known (m, n).  One product per output: the expected value is exact."""
    if gen == "blocks":
        o = P4.operands("blocks", M, N, K)
        A = (o["A"].float() * torch.pow(2.0, ((7 * torch.arange(M)) % 11 - 5).float())[:, None]).to(BF16)
        W4, s, Wp, b, r = o["W4"], o["s"], o["Wp"], None, None
    else:
        o = G.operands(gen, M, N, K, bias, res, swiglu=swiglu)
        A, b, r = o["A"], o["bias"], o["res"]
        W4, s = quantize_blocks_mxfp4(o["W"])
        Wp = dequantize_blocks_mxfp4(W4, s)
    A8, sa = quantize_blocks_mxfp8(A)
    Ap = dequantize_blocks_mxfp8(A8, sa)
    if gen in ("exact", "blocks"):
        assert torch.equal(Ap, A), "small integers and powers of two survive the quantiser"
    return dict(A8=A8, sa=sa, Ap=Ap, W4=W4, s=s, Wp=Wp, bias=b, res=r)


def _case(M, N, K, gen="iid", bias=False, res=False, act=0, force=None, ld=False, norm=None, inplace=False, note=""):
    c = dict(kind="mx", M=M, N=N, K=K, gen=gen, bias=bias, res=res, act=act, force=force or None, ld=ld, norm=norm, inplace=inplace, note=note)
    p = plan_mx(M, N, K, act=act, norm=norm is not None, env=force)
    tag = f"{p['kernel']}-s{p['splits']}" + ("-forced" if force else "")
    ep = ("b" if bias else "") + ("r" if res else "") + ("R" if inplace else "") + (f"a{act}" if act else "") + (f"-{norm}" if norm else "")
    c["id"] = f"mx-{M}x{N}x{K}-{tag}-{gen}" + (f"-{ep}" if ep else "") + ("-ld" if ld else "") + (f"-{note}" if note else "")
    return c


def cases():
    C = []
    add = lambda *a, **k: C.append(_case(*a, **k))
    # --- the four layer GEMMs at the 7B widths, M = 290, with the epilogue the engine gives them (64 reference columns each)
    Hd, I, qd, kd = P4.MODELS["7b"]
    add(290, qd + 2 * kd, Hd, bias=True, note="7b-qkv")
    add(290, Hd, qd, inplace=True, norm="rms", note="7b-o")
    add(290, I, Hd, act=4, note="7b-gateup")
    add(290, Hd, I, res=True, norm="rms", note="7b-down")
    # --- both tile heights x split counts 1, 2, 3 x M in {1, 17, 33, 129, 290} x N in {128, 132, 264} x K in {128, 384, 1536}, forced
    for bm in (64, 128):
        f = lambda s=0: {"SVLM_GEMM_MX_BM": str(bm), **({"SVLM_GEMM_MX_SPLITS": str(s)} if s else {})}
        add(1, 128, 128, gen="blocks", force=f(1))
        add(17, 132, 384, gen="blocks", force=f(3))
        add(33, 264, 1536, gen="blocks", force=f(2))
        add(129, 132, 1536, gen="blocks", force=f(3))
        add(290, 264, 384, gen="blocks", force=f(1))
        add(129, 264, 384, gen="exact", bias=True, res=True, force=f(2))             # kps = 256: the second split is shorter
        add(290, 132, 1536, gen="iid", bias=True, inplace=True, force=f(3))
        add(33, 128, 1536, gen="spread", bias=True, res=True, force=f(1))
        add(17, 264, 128, gen="iid", ld=True, force=f(1))
        add(290, 264, 1536, gen="iid", res=True, ld=True, force=f(2))
        add(129, 132, 384, gen="blocks", ld=True, force=f(3))
        add(129, 264, 1536, gen="iid", bias=True, act=4, force=f(1), note="swiglu")
        add(33, 264, 384, gen="iid", act=4, ld=True, force=f(1), note="swiglu")
        add(290, 264, 1536, gen="iid", res=True, norm="rms", force=f(3), note="norm-in-reduce")
        add(17, 264, 384, gen="iid", inplace=True, norm="rms", ld=True, force=f(2), note="norm-in-reduce")
        add(129, 132, 1536, gen="iid", bias=True, act=3, force=f(2), note="silu")
    # --- by the plan's own rules (these also run on the product library): un-split, split by the grid rule, the norm's two splits,
    # the un-fused norm (K = 128 cannot split), the 128-row tiles from 1024 rows on
    add(290, 132, 1536, gen="iid", bias=True)
    add(17, 128, 384, gen="blocks")
    add(33, 264, 1536, gen="blocks")
    add(290, 264, 384, gen="spread", res=True, norm="rms")
    add(129, 264, 128, gen="iid", inplace=True, norm="rms", note="unfused-norm")
    add(1025, 132, 384, gen="exact", bias=True, res=True, note="128-row-rule")
    add(290, 1024, 256, bias=True, note="tiny-qkv")
    add(290, 512, 256, act=4, note="tiny-gateup")
    return C


CASES = cases()
# the cases the torch emulation of the tile loop runs (tests/test_prefill_mx_host.py)
SMALL_BLOCKS = [c for c in CASES if c["gen"] == "blocks"]
