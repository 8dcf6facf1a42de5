"""Python mirror of the weight-fp8 GEMM's dispatch (gemm_wfp8_impl in csrc/gemm_wfp8.hip, planned by gemm_wcode_plan of csrc/gemm_plan.h) and the case list of
tests/test_gemm_wfp8_gpu.py (test helper, not product; needs no GPU).  Operand generators and the bf16 mirror: tests/gemm_paths.py."""
from __future__ import annotations

import gemm_paths as G

WS_BYTES = G.WS_BYTES
TUNED = G.WCODE_TUNED          # the table of gemm_wcode_plan (csrc/gemm_plan.h)
KERNELS = {64: "wfp8<2,3>", 128: "wfp8<4,3>", 256: "wfp8<4,3,4>"}
_cdiv = G._cdiv


def plan_wfp8(M, N, K, act=0, norm=False, env=None, ws_bytes=WS_BYTES):
    """-> dict(fp8=2, bm, waves, stages, dma, splits, kps, table, norm_fused, kernel).  N = output columns (SwiGLU: I)."""
    return G.plan_wcode("SVLM_GEMM_WFP8", 2, KERNELS, M, N, K, act=act, norm=norm, env=env, ws_bytes=ws_bytes)


def _case(M, N, K, gen="iid", bias=False, res=False, act=0, force=None, ld=False, norm=None, inplace=False, note=""):
    c = dict(kind="wfp8", M=M, N=N, K=K, gen=gen, bias=bias, res=res, act=act, force=force or None, ld=ld, norm=norm, inplace=inplace, note=note)
    p = plan_wfp8(M, N, K, act=act, norm=norm is not None, env=force)
    tag = f"{p['kernel']}-s{p['splits']}" + ("-forced-" + "".join(k.split("_")[-1] + v for k, v in sorted(force.items())) if force else "")
    ep = ("b" if bias else "") + ("r" if res else "") + ("R" if inplace else "") + (f"a{act}" if act else "") + (f"-{norm}" if norm else "")
    c["id"] = f"wfp8-{M}x{N}x{K}-{tag}-{gen}" + (f"-{ep}" if ep else "") + ("-ld" if ld else "") + (f"-{note}" if note else "")
    return c


# (hidden, intermediate, q width, kv width): Qwen2-VL-2B, Qwen2-VL-7B, Qwen2.5-VL-3B
MODELS = {"2b": (1536, 8960, 1536, 256), "7b": (3584, 18944, 3584, 512), "3b": (2048, 11008, 2048, 256)}


def cases():
    C = []
    add = lambda *a, **k: C.append(_case(*a, **k))
    # --- every prefill shape of the three models, with the epilogue the engine gives it
    for name, (Hd, I, qd, kd) in MODELS.items():
        for M in (275, 290, 590):
            add(M, qd + 2 * kd, Hd, bias=True, note=f"{name}-qkv")
            add(M, Hd, qd, inplace=True, norm="rms", note=f"{name}-o")
            add(M, I, Hd, act=4, note=f"{name}-gateup")
            add(M, Hd, I, res=True, norm="rms", note=f"{name}-down")
    # --- tile edges of every tile height (forced where the plan would not put that tile on such an M), un-split and split
    for bm in (64, 128, 256):
        for M_ in (bm - 1, bm, bm + 1):
            add(M_, 260, 1024, gen="rowcol", force={"SVLM_GEMM_WFP8_BM": str(bm)}, note=f"edge{bm}")
            add(M_, 260, 1024, gen="exact", force={"SVLM_GEMM_WFP8_BM": str(bm), "SVLM_GEMM_WFP8_SPLITS": "2"}, note=f"edge{bm}")
    # --- ragged N, by the cost model
    add(275, 2052, 1536, gen="exact")
    add(275, 1540, 1536, gen="spread", bias=True, res=True)
    add(64, 260, 4096, gen="iid", bias=True, act=3, note="splitK-silu-raggedN")
    add(130, 520, 256, gen="iid", bias=True, act=4, note="swiglu-raggedN-bias")
    for act in (1, 2):
        add(200, 388, 1024, gen="iid", bias=True, act=act)
    # --- padded leading dimensions: un-split, split, split + fused norm, SwiGLU
    add(275, 2052, 512, gen="exact", bias=True, res=True, ld=True)
    add(290, 1536, 8960, gen="exact", bias=True, res=True, ld=True)
    add(290, 1536, 8960, gen="iid", res=True, norm="rms", ld=True)
    add(130, 520, 256, gen="iid", act=4, ld=True)
    # --- one 4096-row pass (256-row tiles) and the 128-row leg of the large-M rule
    add(4096, 3584, 3584, gen="exact", bias=True, res=True, note="dense-o")
    add(2305, 3460, 2048, gen="rowcol", note="largeM-128")
    # --- the tiny widths
    add(290, 1024, 256, bias=True, note="tiny-qkv")
    add(290, 256, 512, inplace=True, norm="rms", note="tiny-o-unfused-norm")
    add(290, 512, 256, act=4, note="tiny-gateup")
    add(33, 256, 512, gen="spread", res=True, norm="rms", note="tiny-down")
    # --- every instantiation forced at one ragged shape (M not a multiple of the tile rows, N = 128 j + 4, kps not dividing K)
    M, N, K = 333, 388, 1984
    for bm in (64, 128, 256):
        env = {"SVLM_GEMM_WFP8_BM": str(bm)}
        add(M, N, K, gen="exact", force=dict(env))
        add(M, N, K, gen="rowcol", force=dict(env))
        add(M, N, K, gen="exact", bias=True, inplace=True, force=dict(env))
        add(M, 392, K, gen="iid", act=4, force=dict(env))
        env["SVLM_GEMM_WFP8_SPLITS"] = "3"
        add(M, N, K, gen="exact", bias=True, inplace=True, force=dict(env))
        add(M, N, K, gen="iid", bias=True, res=True, act=3, force=dict(env))
        add(M, 392, K, gen="iid", res=True, norm="rms", force=dict(env))
    return C


CASES = cases()
