"""Python mirror of the weight-fp4 GEMM's dispatch (gemm_wfp4_impl in csrc/gemm_wfp4.hip, planned by gemm_wcode_plan of csrc/gemm_plan.h), the operand builder and the case list of
tests/test_gemm_wfp4_gpu.py (test helper, not product; needs no GPU).  Operand generators and the bf16 mirror: tests/gemm_paths.py."""
from __future__ import annotations

import torch

import gemm_paths as G

from streaming_vlm_amd.weights import dequantize_blocks_mxfp4, quantize_blocks_mxfp4

BF16 = torch.bfloat16
WS_BYTES = G.WS_BYTES
TUNED = G.WCODE_TUNED          # the table of gemm_wcode_plan (csrc/gemm_plan.h)
KERNELS = {64: "wfp4<2,2>", 128: "wfp4<4,2>", 256: "wfp4<4,4>"}
_cdiv = G._cdiv


def plan_wfp4(M, N, K, act=0, norm=False, env=None, ws_bytes=WS_BYTES):
    """-> dict(fp8=3, bm, waves, stages, dma, splits, kps, table, norm_fused, kernel).  N = output columns (SwiGLU: I)."""
    return G.plan_wcode("SVLM_GEMM_WFP4", 3, KERNELS, M, N, K, act=act, norm=norm, env=env, ws_bytes=ws_bytes)


def operands(gen, M, N, K, bias=False, res=False, swiglu=False):
    """gemm_paths.operands with W quantised to MXFP4 -> dict(A, W4 (Nw, K / 2) uint8, s (Nw, K / 32) uint8, Wp = W' (Nw, K) bf16, the
    matrix the reference multiplies by, bias, res), on the CPU.
    blocks: A one-hot in k per row as in `rowcol` (k = (37 m + 5) % K), rowcol's W pre-scaled per (row n, block b) by
            2^((5 n + 3 b) % 9 - 4) before quantisation: neighbouring blocks (3), rows (5) and K-tiles (6) carry different scale
            bytes, so a scale taken from the wrong block, row, K-tile or split offset shows as a wrong value at a known (m, n)."""
    if gen == "blocks":
        assert not swiglu and not bias and not res
        o = G.operands("rowcol", M, N, K)
        n, b = torch.arange(N), torch.arange(K // 32)
        f = torch.pow(2.0, ((5 * n[:, None] + 3 * b[None, :]) % 9 - 4).float())
        o["W"] = (o["W"].float().view(N, K // 32, 32) * f[:, :, None]).view(N, K).to(BF16)
    else:
        o = G.operands(gen, M, N, K, bias, res, swiglu=swiglu)
    W4, s = quantize_blocks_mxfp4(o["W"])
    Wp = dequantize_blocks_mxfp4(W4, s)
    if gen == "exact":
        assert torch.equal(Wp, o["W"]), "0/1 weights survive the quantiser"
    return dict(A=o["A"], W4=W4, s=s, Wp=Wp, bias=o["bias"], res=o["res"])


def _case(M, N, K, gen="iid", bias=False, res=False, act=0, force=None, ld=False, norm=None, inplace=False, note=""):
    c = dict(kind="wfp4", M=M, N=N, K=K, gen=gen, bias=bias, res=res, act=act, force=force or None, ld=ld, norm=norm, inplace=inplace, note=note)
    p = plan_wfp4(M, N, K, act=act, norm=norm is not None, env=force)
    tag = f"{p['kernel']}-s{p['splits']}" + ("-forced-" + "".join(k.split("_")[-1] + v for k, v in sorted(force.items())) if force else "")
    ep = ("b" if bias else "") + ("r" if res else "") + ("R" if inplace else "") + (f"a{act}" if act else "") + (f"-{norm}" if norm else "")
    c["id"] = f"wfp4-{M}x{N}x{K}-{tag}-{gen}" + (f"-{ep}" if ep else "") + ("-ld" if ld else "") + (f"-{note}" if note else "")
    return c


# (hidden, intermediate, q width, kv width): Qwen2-VL-2B, Qwen2-VL-7B, Qwen2.5-VL-3B
MODELS = {"2b": (1536, 8960, 1536, 256), "7b": (3584, 18944, 3584, 512), "3b": (2048, 11008, 2048, 256)}
WIDE = 3584          # cases of this width and above check the fp64 reference on ref_columns() only


def ref_columns(case):
    """The output columns the fp64 reference covers: all of them, or (7B widths) 64 that include the first, the last and both sides of
    the first and the last tile edge; bit-equality with the bf16 twin covers the whole output."""
    N = case["N"]
    if max(N, case["K"]) < WIDE:
        return None
    bn = 64 if case["act"] == 4 else 128
    last_edge = (N - 1) // bn * bn
    cols = set(range(0, 8)) | set(range(bn - 8, bn + 8)) | set(range(last_edge - 8, last_edge + 8)) | set(range(N - 8, N))
    mid = N // 2 // bn * bn
    cols |= set(range(mid - 4, mid + 4))
    cols = sorted(c for c in cols if 0 <= c < N)
    assert len(cols) <= 64 and cols[0] == 0 and cols[-1] == N - 1
    return cols


def cases():
    C = []
    add = lambda *a, **k: C.append(_case(*a, **k))
    # --- every prefill shape of the three models at M = 290, with the epilogue the engine gives it; the 7B shapes at M = 590 where
    # the table has an entry of its own (down_proj, gate/up)
    for name, (Hd, I, qd, kd) in MODELS.items():
        add(290, qd + 2 * kd, Hd, bias=True, note=f"{name}-qkv")
        add(290, Hd, qd, inplace=True, norm="rms", note=f"{name}-o")
        add(290, I, Hd, act=4, note=f"{name}-gateup")
        add(290, Hd, I, res=True, norm="rms", note=f"{name}-down")
    add(590, 18944, 3584, act=4, note="7b-gateup")
    add(590, 3584, 18944, res=True, norm="rms", note="7b-down")
    # --- tile edges of every tile height (forced where the plan would not put that tile on such an M), un-split and split
    for bm in (64, 128, 256):
        for M_ in (bm - 1, bm, bm + 1):
            add(M_, 260, 1024, gen="blocks", force={"SVLM_GEMM_WFP4_BM": str(bm)}, note=f"edge{bm}")
            add(M_, 260, 1024, gen="exact", force={"SVLM_GEMM_WFP4_BM": str(bm), "SVLM_GEMM_WFP4_SPLITS": "2"}, note=f"edge{bm}")
        add(bm + 1, 260, 1024, gen="blocks", force={"SVLM_GEMM_WFP4_BM": str(bm), "SVLM_GEMM_WFP4_SPLITS": "2"}, note=f"edge{bm}")
    # --- ragged N, by the cost model
    add(275, 2052, 1536, gen="exact")
    add(275, 1540, 1536, gen="spread", bias=True, res=True)
    add(64, 260, 4096, gen="iid", bias=True, act=3, note="splitK-silu-raggedN")
    add(64, 260, 4096, gen="blocks", note="splitK-raggedN")
    add(130, 520, 256, gen="iid", bias=True, act=4, note="swiglu-raggedN-bias")
    for act in (1, 2):
        add(200, 388, 1024, gen="iid", bias=True, act=act)
    # --- padded leading dimensions (A, W4, C, residual, XN): un-split, split, split + fused norm, SwiGLU
    add(275, 2052, 512, gen="exact", bias=True, res=True, ld=True)
    add(290, 1536, 8960, gen="exact", bias=True, res=True, ld=True)
    add(290, 1536, 8960, gen="iid", res=True, norm="rms", ld=True)
    add(275, 388, 1536, gen="blocks", ld=True)
    add(130, 520, 256, gen="iid", act=4, ld=True)
    # --- one 4096-row pass (256-row tiles) and the 128-row leg of the large-M rule
    add(4096, 3584, 3584, gen="exact", bias=True, res=True, note="dense-o")
    add(2305, 3460, 2048, gen="blocks", note="largeM-128")
    # --- the tiny widths
    add(290, 1024, 256, bias=True, note="tiny-qkv")
    add(290, 256, 512, inplace=True, norm="rms", note="tiny-o-unfused-norm")
    add(290, 512, 256, act=4, note="tiny-gateup")
    add(33, 256, 512, gen="spread", res=True, norm="rms", note="tiny-down")
    # --- every instantiation forced at one ragged shape (M not a multiple of the tile rows, N = 128 j + 4, kps = 704 not dividing K,
    # so that k_begin is no multiple of the table's K per split)
    M, N, K = 333, 388, 1984
    for bm in (64, 128, 256):
        env = {"SVLM_GEMM_WFP4_BM": str(bm)}
        add(M, N, K, gen="blocks", force=dict(env))
        add(M, N, K, gen="exact", bias=True, inplace=True, force=dict(env))
        add(M, 392, K, gen="iid", act=4, force=dict(env))
        env["SVLM_GEMM_WFP4_SPLITS"] = "3"
        add(M, N, K, gen="blocks", force=dict(env))
        add(M, N, K, gen="exact", bias=True, inplace=True, force=dict(env))
        add(M, N, K, gen="iid", bias=True, res=True, act=3, force=dict(env))
        add(M, 392, K, gen="iid", res=True, norm="rms", force=dict(env))
    return C


CASES = cases()
# the cases the torch emulation of the tile loop runs (tests/test_prefill_fp4_host.py): `blocks` on small shapes
SMALL_BLOCKS = [c for c in CASES if c["gen"] == "blocks" and c["M"] * c["N"] * c["K"] <= 333 * 388 * 1984]
