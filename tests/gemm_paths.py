"""Python mirror of the GEMM dispatch (gemm_impl in csrc/gemm.hip, gemm_fp8_impl in csrc/gemm_fp8.hip), the operand generators and the
case list of tests/test_gemm_paths_gpu.py (test helper, not product; needs no GPU).

The mirror restates the cost model, the tuned table, the large-M rules and the tuning switches line by line (the pieces the GEMMs share
in csrc/gemm_plan.h once: _cost_plan, _large_m_bm, _finish_split, plan_wcode), so that every case can name the kernel it expects in its id and the GPU test can assert that the diagnostic library reports exactly that plan.  A dispatch
edit that is not mirrored here fails tests/test_gemm_ref64.py::test_mirror_matches_the_library_plan without a GPU."""
from __future__ import annotations

import torch

BF16 = torch.bfloat16
WS_BYTES = 96 << 20            # HipOps.GEMM_WS_BYTES

# (mb, N, K, bm, splits, variant) -- kTunedPlans of gemm.hip
TUNED = [(5, 1536, 8960, 64, 4, 0), (5, 4608, 3584, 64, 2, 0), (5, 3584, 3584, 64, 3, 0), (5, 3584, 18944, 320, 8, 0),
         (10, 3584, 18944, 128, 3, 0), (10, 18944, 3584, 128, 1, 2), (5, 2560, 2048, 64, 3, 0), (5, 2048, 2048, 64, 3, 0),
         (5, 2048, 11008, 64, 4, 0), (16, 3840, 1280, 128, 1, 1), (16, 1280, 5120, 128, 3, 0), (16, 1280, 1280, 128, 3, 0),
         (16, 1280, 3424, 128, 3, 0), (4, 5120, 5120, 128, 3, 0), (4, 1536, 5120, 64, 5, 0), (4, 3584, 5120, 128, 4, 0),
         (4, 2048, 5120, 64, 4, 0)]

# every kernel instantiation -> the forms (split K or not) the PRODUCT dispatch can reach it in
KERNELS = {
    "reg<2>": {"unsplit", "split"},
    "reg<4>": {"unsplit", "split"},           # split: table entry (16, 1280, 3424): K % 64 == 32 (Qwen2.5 ViT down_proj)
    "glds<2,2>": {"unsplit"},                 # un-split 64-row tiles only
    "glds<2,3>": {"split"},                   # un-split needs SVLM_GEMM_NS3
    "glds<4,2>": {"unsplit"},
    "glds<4,3>": {"unsplit", "split"},
    "glds<2,3,4>": {"unsplit"},               # 128 rows on 8 waves: table entry only
    "glds<4,3,4>": {"unsplit"},               # 256 rows: the large-M rule needs an un-split plan
    "glds<6,3>": set(),                       # 192 rows: switch only
    "glds<10,2>": {"split"},                  # 320 rows: table entry only (8 splits)
    "fp8<2,3>": {"unsplit", "split"},
    "fp8<4,3>": set(),                        # switch only
}
FORCE_BM = {"reg<2>": 64, "reg<4>": 128, "glds<2,2>": 64, "glds<2,3>": 64, "glds<4,2>": 128, "glds<4,3>": 128, "glds<2,3,4>": 128,
            "glds<4,3,4>": 256, "glds<6,3>": 192, "glds<10,2>": 320}


def _cdiv(a, b):
    return (a + b - 1) // b


def _cost_plan(M, N, K, gn, ws_bytes):
    """gemm_cost_plan (csrc/gemm_plan.h) -> (bm, splits)"""
    best_bm, best_splits, best_cost = 64, 1, 1e30
    for bm_c in (64, 128):
        if bm_c == 128 and M <= 64:
            continue
        tiles_c = _cdiv(M, bm_c) * gn
        cap = 256 * (3 if bm_c == 64 else 2)
        max_s = (min(K // 512, 16) if K >= 1024 else 1)
        for sp in range(1, max_s + 1):
            if sp > 1 and sp * M * N * 4 > ws_bytes:
                break
            wgs = tiles_c * sp
            rounds = float((wgs + cap - 1) // cap)
            ksteps = float((K + sp - 1) // sp + 63) / 64 + 3.0
            step_us = 0.9 if bm_c == 64 else 1.5
            slab_us = (2.0 * sp * M * N * 4.0 / 3e12 * 1e6 + 5.0) if sp > 1 else 0.0
            cost = rounds * ksteps * step_us + slab_us
            if cost < best_cost:
                best_cost, best_bm, best_splits = cost, bm_c, sp
    return best_bm, best_splits


def _large_m_bm(M, gn):
    """gemm_large_m_bm (csrc/gemm_plan.h)"""
    t256 = _cdiv(M, 256) * gn
    rounds = (t256 + 255) // 256
    return 256 if t256 * 100 >= rounds * 256 * 85 else 128


def _finish_split(K, bk, splits):
    """gemm_finish_split (csrc/gemm_plan.h) -> (splits, kps)"""
    if splits <= 1:
        return splits, K
    kps = _cdiv(_cdiv(K, splits), bk) * bk
    return _cdiv(K, kps), kps


# (mb, N, K, bm, splits) -- kPlans of gemm_wcode_plan (csrc/gemm_plan.h)
WCODE_TUNED = [(5, 1536, 8960, 64, 4), (5, 4608, 3584, 64, 2), (5, 3584, 3584, 64, 3), (5, 3584, 18944, 128, 8), (10, 3584, 18944, 128, 3),
               (10, 18944, 3584, 128, 1), (5, 2560, 2048, 64, 3), (5, 2048, 2048, 64, 3), (5, 2048, 11008, 64, 4)]


def plan_wcode(prefix, kind, kernels, M, N, K, act=0, norm=False, env=None, ws_bytes=WS_BYTES):
    """gemm_wcode_plan (csrc/gemm_plan.h), the plan of the weight-code GEMMs -> dict(fp8=kind, bm, waves, stages, dma, splits, kps,
    table, norm_fused, kernel).  prefix: of the switch names; kernels: {tile rows: kernel name}; N = output columns (SwiGLU: I)."""
    env = env or {}
    swiglu = act == 4
    gn = _cdiv(N, 64) if swiglu else _cdiv(N, 128)
    best_bm, best_splits = _cost_plan(M, N, K, gn, ws_bytes)
    table = False
    if prefix + "_NO_TABLE" not in env:
        mb = _cdiv(M, 64)
        for (pmb, pN, pK, pbm, psp) in WCODE_TUNED:
            if pN == N and pK == K and pmb - 1 <= mb <= pmb + 1 and (psp == 1 or psp * M * N * 4 <= ws_bytes):
                best_bm, best_splits, table = pbm, psp, True
                break
    if M >= 2048 and K >= 2048 and best_splits == 1:
        best_bm = _large_m_bm(M, gn)
    if prefix + "_BM" in env:
        fb = int(env[prefix + "_BM"])
        best_bm = fb if fb in (128, 256) else 64
        table = False
        fs = int(env.get(prefix + "_SPLITS", "0"))
        best_splits = fs if fs > 0 else 1
        if best_splits * M * N * 4 > ws_bytes or K < 1024:
            best_splits = 1
    if swiglu:
        best_splits = 1
    bm = best_bm
    splits, kps = _finish_split(K, 64, best_splits)
    return dict(fp8=kind, bm=bm, waves=8 if bm == 256 else 4, stages=3, dma=1, splits=splits, kps=kps, table=int(table),
                norm_fused=int(bool(norm) and splits > 1 and N <= 4096), kernel=kernels[bm])


def plan_bf16(M, N, K, act=0, norm=False, env=None, ws_bytes=WS_BYTES):
    """-> dict(fp8, bm, waves, stages, dma, splits, kps, table, norm_fused, kernel).  N = output columns (SwiGLU: I)."""
    env = env or {}
    swiglu = act == 4
    gn = _cdiv(N, 64) if swiglu else _cdiv(N, 128)
    best_bm, best_splits = _cost_plan(M, N, K, gn, ws_bytes)
    plan_w8 = plan_ns2 = table = False
    if "SVLM_GEMM_NO_TABLE" not in env:
        mb = _cdiv(M, 64)
        for (pmb, pN, pK, pbm, psp, pvar) in TUNED:
            if pN == N and pK == K and pmb - 1 <= mb <= pmb + 1 and (psp == 1 or psp * M * N * 4 <= ws_bytes):
                best_bm, best_splits, plan_w8, plan_ns2, table = pbm, psp, pvar == 1, pvar == 2, True
                break
    dma = K % 64 == 0 and "SVLM_GEMM_NO_DMA" not in env
    if dma and M >= 2048 and K >= 2048 and best_splits == 1 and "SVLM_GEMM_NO_T128" not in env:
        best_bm = _large_m_bm(M, gn)
    if "SVLM_GEMM_BM" in env:
        fb = int(env["SVLM_GEMM_BM"])
        best_bm = fb if fb in (192, 320, 256) else (128 if fb == 128 and M > 64 else 64)
        plan_w8 = plan_ns2 = table = False
        fs = int(env.get("SVLM_GEMM_SPLITS", "0"))
        best_splits = fs if fs > 0 else 1
        if best_splits * M * N * 4 > ws_bytes or K < 1024:
            best_splits = 1
    if swiglu:
        best_splits = 1
        if best_bm > 128 and best_bm != 256:
            best_bm = 128
    bm = best_bm
    splits, kps = _finish_split(K, 64, best_splits)
    if not dma and (bm in (192, 320, 256) or swiglu):
        raise ValueError("tall tiles and SwiGLU need the LDS-DMA kernel")
    small = bm == 64
    if not dma:
        kernel, waves, stages = ("reg<2>" if small else "reg<4>"), 4, 2
    elif bm == 128 and splits == 1 and not swiglu and (plan_w8 or "SVLM_GEMM_W8" in env):
        kernel, waves, stages = "glds<2,3,4>", 8, 3
    elif bm == 256:
        kernel, waves, stages = "glds<4,3,4>", 8, 3
    elif bm == 192:
        kernel, waves, stages = "glds<6,3>", 4, 3
    elif bm == 320:
        kernel, waves, stages = "glds<10,2>", 4, 2
    elif small and splits == 1 and "SVLM_GEMM_NS3" not in env:
        kernel, waves, stages = "glds<2,2>", 4, 2
    elif not small and splits == 1 and (M >= 2048 or plan_ns2 or "SVLM_GEMM_T128NS2" in env):
        kernel, waves, stages = "glds<4,2>", 4, 2
    elif small:
        kernel, waves, stages = "glds<2,3>", 4, 3
    else:
        kernel, waves, stages = "glds<4,3>", 4, 3
    return dict(fp8=0, bm=bm, waves=waves, stages=stages, dma=int(dma), splits=splits, kps=kps, table=int(table),
                norm_fused=int(bool(norm) and splits > 1 and N <= 4096), kernel=kernel)


def plan_fp8(M, N, K, norm=False, env=None, ws_bytes=WS_BYTES):
    env = env or {}
    gn = _cdiv(N, 128)
    bm, splits = 64, 1
    tiles = _cdiv(M, bm) * gn
    if tiles < 160 and K >= 1024:
        splits = min((256 + tiles - 1) // tiles, K // 512, 8)
        while splits > 1 and splits * M * N * 4 > ws_bytes:
            splits -= 1
    if "SVLM_GEMM8_SPLITS" in env:
        v = int(env["SVLM_GEMM8_SPLITS"])
        if v >= 1 and (v == 1 or v * M * N * 4 <= ws_bytes):
            splits = v
    if "SVLM_GEMM8_BM" in env and int(env["SVLM_GEMM8_BM"]) in (64, 128):
        bm = int(env["SVLM_GEMM8_BM"])
    if norm and splits == 1 and K >= 1024 and 2 * M * N * 4 <= ws_bytes and N <= 4096:
        splits = 2
    splits, kps = _finish_split(K, 128, splits)
    return dict(fp8=1, bm=bm, waves=4, stages=3, dma=1, splits=splits, kps=kps, table=0,
                norm_fused=int(bool(norm) and splits > 1 and N <= 4096), kernel="fp8<2,3>" if bm == 64 else "fp8<4,3>")


def plan_of(case, forced=False):
    env = case["force"] if forced else None
    if case["kind"] == "fp8":
        return plan_fp8(case["M"], case["N"], case["K"], norm=case["norm"] is not None, env=env)
    return plan_bf16(case["M"], case["N"], case["K"], act=case["act"], norm=case["norm"] is not None, env=env)


# ------------------------------------------------------------------------------------------------------------ operand generators
def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def operands(gen, M, N, K, bias=False, res=False, swiglu=False):
    """-> dict(A (M, K), W (Nw, K), bias (Nw,) | None, res (M, N) | None), bf16 on the CPU; Nw = 2 N for SwiGLU.
    iid:    randn operands (the shapes' usual scales).
    spread: iid with the rows of A scaled by 2^-6 .. 2^6, so small outputs sit next to large ones.
    exact:  W[n, k] = 1 where k % 128 == n % 128, A[m, k] = (m + k + k // 128) % 3 - 1: every partial sum is a small integer, every
            k-column feeds some output column, so the output equals the reference bit for bit on every path; bias / residual are small
            integers.  Along the k that feed one output (k = n % 128 + 128 j) A is CONSTANT, (m + n) % 3 - 1, since 129 % 3 == 0: the
            output is that constant times K / 128, so nothing cancels and a dropped or doubled K-slice of any length moves two
            outputs in three.
    rowcol: A one-hot in k per row (k = (37 m + 5) % K), W[n, k] = (131 n + 7 k) % 251 - 125: the output is the gather W[n, k(m)], a
            transposed fragment, swapped row block or mis-addressed tile column shows as a wrong code at a known (m, n)."""
    Nw = 2 * N if swiglu else N
    if gen in ("iid", "spread"):
        A, W = _randn((M, K), 1), _randn((Nw, K), 2, 0.05)
        if gen == "spread":
            A = (A.float() * (2.0 ** ((torch.arange(M) % 13) - 6).float())[:, None]).to(BF16)
        b = _randn((Nw,), 3, 0.1) if bias else None
        r = _randn((M, N), 4) if res else None
    elif gen == "exact":
        assert not swiglu
        k, n, m = torch.arange(K), torch.arange(Nw), torch.arange(M)
        W = ((k[None, :] % 128) == (n[:, None] % 128)).to(BF16)
        A = (((m[:, None] + k[None, :] + k[None, :] // 128) % 3) - 1).to(BF16)
        b = ((n % 5) - 2).to(BF16) if bias else None
        r = (((m[:, None] + 2 * n[None, :]) % 7) - 3).to(BF16) if res else None
    elif gen == "rowcol":
        assert not swiglu
        k, n, m = torch.arange(K), torch.arange(Nw), torch.arange(M)
        A = torch.zeros((M, K), dtype=BF16)
        A[m, (37 * m + 5) % K] = 1
        W = (((131 * n[:, None] + 7 * k[None, :]) % 251) - 125).to(BF16)
        b = r = None
        assert not bias and not res
    else:
        raise ValueError(gen)
    return dict(A=A, W=W, bias=b, res=r)


# ------------------------------------------------------------------------------------------------------------ the case list
def _case(kind, M, N, K, gen="iid", bias=False, res=False, act=0, force=None, ld=False, norm=None, inplace=False, note=""):
    c = dict(kind=kind, M=M, N=N, K=K, gen=gen, bias=bias, res=res, act=act, force=force or None, ld=ld, norm=norm, inplace=inplace, note=note)
    p = plan_of(c)
    tag = f"{p['kernel']}-s{p['splits']}"
    if force:
        pf = plan_of(c, forced=True)
        tag += f"-forced-{pf['kernel']}-s{pf['splits']}-" + "".join(k.split("_")[-1] + v for k, v in sorted(force.items()))
    ep = ("b" if bias else "") + ("r" if res else "") + ("R" if inplace else "") + (f"a{act}" if act else "") + (f"-{norm}" if norm else "")
    c["id"] = f"{kind}-{M}x{N}x{K}-{tag}-{gen}" + (f"-{ep}" if ep else "") + ("-ld" if ld else "") + (f"-{note}" if note else "")
    return c


def _bf16_cases():
    C = []
    add = lambda *a, **k: C.append(_case("bf16", *a, **k))
    # --- unforced: every product-reachable (kernel, split?) pair, incl. the ones no other test shape reaches
    add(1024, 1284, 1176, gen="exact")                             # reg<2> unsplit? (patch embed's K, ragged N)
    add(70, 132, 1176, gen="exact", note="reg64-splitK-tail")      # reg<2> split-K with a K tail (K >= 1024, K % 64 != 0, small M)
    add(70, 132, 1176, gen="iid", bias=True, res=True, act=3)
    add(200, 128, 1000, gen="exact")                               # K < 1024: does NOT split
    add(1000, 6200, 200, gen="rowcol")                             # reg<4> unsplit (784 64-row tiles > 768 resident)
    add(1000, 6200, 200, gen="iid", bias=True)
    add(1000, 1284, 1176, gen="spread", bias=True, res=True)
    add(2100, 3460, 2056, gen="exact", note="largeM-K-not-64")     # the large-M rule must not hand a K % 64 != 0 GEMM to the DMA-only tile
    add(1024, 1280, 3424, gen="exact", note="reg128-splitK")       # reg<4> split 3, kps 1152, K tail 1120: table entry, K % 64 == 32
    add(1000, 1280, 3424, gen="iid", bias=True, res=True)          # ... ragged M
    add(961, 1280, 3424, gen="rowcol", note="bucket-low")          # the entry's row bucket: mb 15..17
    add(1088, 1280, 3424, gen="spread", bias=True, res=True, act=1, note="bucket-high")
    add(1000, 6200, 192, gen="rowcol")                             # glds<4,3> unsplit (M < 2048, no table entry)
    add(1000, 6200, 192, gen="iid", bias=True, act=1)
    add(2050, 3204, 128, gen="exact")                              # glds<4,2> plain epilogue (M >= 2048, K < 2048), ragged M and N
    add(2050, 3204, 128, gen="iid", bias=True, res=True)
    add(275, 2052, 1536, gen="exact")                              # glds<2,2> / glds<2,3> by the cost model
    add(275, 1540, 1536, gen="iid", res=True)
    add(64, 260, 4096, gen="iid", bias=True, act=3, note="splitK-silu-raggedN")
    add(64, 260, 4096, gen="exact")
    add(1000, 3840, 1280, gen="iid", bias=True)                    # glds<2,3,4> (table), ragged M
    add(1000, 3840, 1280, gen="rowcol")
    add(1024, 1280, 1280, gen="spread", bias=True, res=True)       # glds<4,3> split 3 (table)
    add(256, 3584, 5120, gen="exact", bias=True)                   # glds<4,3> split 4 (table)
    add(290, 1536, 8960, gen="exact", res=True)                    # glds<2,3> split 4 (table)
    add(290, 1536, 8960, gen="iid", bias=True, res=True)
    add(590, 3584, 18944, gen="exact")                             # glds<4,3> split 3 (table)
    # 320-row tile: its table bucket's two ends and the middle
    add(193, 3584, 18944, gen="exact", note="320-bucket-low")
    add(290, 3584, 18944, gen="iid", res=True)
    add(384, 3584, 18944, gen="exact", res=True, note="320-bucket-high-2nd-tile-64-rows")
    add(321, 3584, 18944, gen="rowcol", note="320+1")
    add(320, 3584, 18944, gen="rowcol", note="320")
    add(319, 3584, 18944, gen="rowcol", note="320-1")
    # 256-row tile (large-M rule): ragged M and N, tile edges
    add(2048, 3584, 3584, gen="exact", bias=True, res=True)
    add(2049, 3460, 2048, gen="rowcol", note="256k+1-raggedN")     # 9 row tiles, the last holds one row
    add(2303, 3460, 2048, gen="iid", bias=True, act=2, note="256k-1-raggedN")
    add(2304, 3460, 2048, gen="exact", note="256k")
    add(2305, 3460, 2048, gen="spread", bias=True, res=True)       # 280 tiles of 256 rows fill 55 % of two rounds: the rule's 128-row leg
    add(2100, 392, 2048, gen="spread", bias=True, res=True)        # large M, few tiles: the cost model splits K instead
    # 128-row tile edges (unforced: glds<4,3> split by table at mb 16 +- 1: M = 961..1088 only; edges forced below)
    # SwiGLU
    add(590, 18944, 3584, gen="iid", act=4)                        # glds<4,2> via table
    add(130, 520, 256, gen="iid", bias=True, act=4)
    add(2048, 1792, 2048, gen="iid", act=4)                        # 256-row SwiGLU
    # --- forced: every instantiation at one ragged shape (M not a multiple of the tile rows, N = 128 j + 4, kps not dividing K)
    M, N, K = 333, 388, 1984
    for kern, bm in FORCE_BM.items():
        env = {"SVLM_GEMM_BM": str(bm)}
        Kc = K + 8 if kern.startswith("reg") else K
        if kern == "glds<2,3>":
            env["SVLM_GEMM_NS3"] = "1"
        if kern == "glds<4,2>":
            env["SVLM_GEMM_T128NS2"] = "1"
        if kern == "glds<2,3,4>":
            env["SVLM_GEMM_W8"] = "1"
        add(M, N, Kc, gen="exact", force=dict(env))                                          # no epilogue, unsplit
        add(M, N, Kc, gen="exact", bias=True, inplace=True, force=dict(env))                 # bias + residual in place
        if kern in ("glds<2,2>", "glds<4,2>", "glds<2,3,4>"):
            continue                                                                        # un-split kernels by construction
        env["SVLM_GEMM_SPLITS"] = "3"
        add(M, N, Kc, gen="exact", force=dict(env))                                          # split with a tail: kps 704 (or 704 of 1992)
        add(M, N, Kc, gen="exact", bias=True, inplace=True, force=dict(env))
        for act in (1, 2, 3):
            add(M, N, Kc, gen="iid", bias=True, act=act, force=dict(env))                    # each activation through the reduce
    # --- tile edges, forced where the product plan does not put that tile on such an M
    for bm, extra in ((128, {}), (192, {}), (256, {}), (320, {})):
        for M_ in (bm - 1, bm, bm + 1):
            add(M_, 260, 1024, gen="rowcol", force={"SVLM_GEMM_BM": str(bm), **extra}, note=f"edge{bm}")
            add(M_, 260, 1024, gen="exact", force={"SVLM_GEMM_BM": str(bm), "SVLM_GEMM_SPLITS": "2", **extra}, note=f"edge{bm}")
    # --- leading dimensions: one split and one unsplit case per kernel family
    for (M_, N_, K_, force) in ((70, 132, 1176, None), (200, 132, 1000, None),                   # register-staged: split, unsplit
                                (1000, 1280, 3424, None),                                         # ... 128 rows, split
                                (275, 1540, 1536, None), (275, 2052, 512, None),                  # DMA 64
                                (1024, 1280, 1280, None), (1000, 6200, 192, None),                # DMA 128
                                (2049, 3460, 2048, None), (300, 260, 1984, {"SVLM_GEMM_BM": "256", "SVLM_GEMM_SPLITS": "3"}),   # 256
                                (290, 3584, 18944, None), (300, 260, 1984, {"SVLM_GEMM_BM": "320"})):                         # 320
        add(M_, N_, K_, gen="exact", bias=True, res=True, ld=True, force=force)
    # --- fused norm
    add(290, 1536, 8960, gen="iid", res=True, norm="rms")
    add(290, 1536, 8960, gen="iid", res=True, norm="rms", ld=True)
    add(1024, 1280, 5120, gen="iid", bias=True, res=True, norm="ln")
    add(1024, 1280, 5120, gen="iid", bias=True, res=True, norm="ln", ld=True)
    add(33, 256, 512, gen="iid", res=True, norm="rms")             # unfused (no split)
    return C


def _fp8_cases():
    C = []
    add = lambda *a, **k: C.append(_case("fp8", *a, **k))
    add(1024, 3844, 1280, gen="iid", bias=True)                                    # 64-row default, unsplit, ragged N
    add(1000, 1028, 1280, gen="iid", bias=True, res=True)                          # split by the tile-count rule, ragged M and N
    add(1000, 1028, 1280, gen="exact")
    add(70, 260, 128, gen="iid", bias=True, res=True, act=3)
    for s in range(1, 9):                                                          # forced splits 1..8 with a tail (K = 4480 = 35 x 128)
        add(333, 388, 4480, gen="exact", bias=True, inplace=True, force={"SVLM_GEMM8_SPLITS": str(s)})
    add(333, 388, 4480, gen="iid", bias=True, act=1, force={"SVLM_GEMM8_SPLITS": "3"})
    add(333, 388, 4480, gen="exact", force={"SVLM_GEMM8_BM": "128"})               # 128-row tile, forced
    add(333, 388, 4480, gen="iid", bias=True, res=True, force={"SVLM_GEMM8_BM": "128", "SVLM_GEMM8_SPLITS": "3"})
    add(129, 132, 1280, gen="rowcol", force={"SVLM_GEMM8_BM": "128"})
    add(1024, 3840, 1280, gen="iid", bias=True, res=True, norm="ln", note="norm-forced-split")      # 240 tiles: unsplit but for the norm rule
    add(1000, 1280, 1280, gen="iid", bias=True, res=True, norm="ln", note="normq")
    add(1000, 1280, 1280, gen="iid", bias=True, res=True, norm="rms", note="normq")
    add(333, 392, 1280, gen="exact", bias=True, res=True, ld=True)
    add(333, 392, 4480, gen="exact", bias=True, res=True, ld=True, force={"SVLM_GEMM8_SPLITS": "1"})
    return C


CASES = _bf16_cases() + _fp8_cases()
