"""GPU parity: every C-ABI kernel against the CPU oracle math (tests/ref_ops.py) on seeded inputs.

Tolerances (stated per test): outputs are bf16, so the bar is "same value up to one bf16 rounding
flip": max |err| <= 2^-7 * max|ref| (one ulp at the top of the range) AND mean |err| <= 1e-3 * max|ref|
(a systematic error of even a tenth of an ulp fails the mean).  Integer / index outputs are exact.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def diag():
    import helpers as H
    return H.diag_ops()


@pytest.fixture(scope="module")
def ref():
    from ref_ops import RefOps
    return RefOps()


def rnd(shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def close(name, got, want, max_tol=2 ** -7, mean_tol=1e-3):
    got = got.detach().float().cpu()
    want = want.detach().float().cpu()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    scale = float(want.abs().max()) + 1e-30
    err = (got - want).abs()
    mx, mean = float(err.max()) / scale, float(err.mean()) / scale
    frac = float((err > 0).float().mean())
    print(f"[{name}] max_err/scale={mx:.3e} mean_err/scale={mean:.3e} mismatched={frac:.4f} scale={scale:.3e}")
    assert mx <= max_tol, f"{name}: max err {mx:.3e} > {max_tol:.3e}"
    assert mean <= mean_tol, f"{name}: mean err {mean:.3e} > {mean_tol:.3e}"


# ----------------------------------------------------------------------------- GEMM / GEMV
@pytest.mark.parametrize("M,N,K,bias,res,act", [
    (1024, 3840, 1280, True, False, 0),     # ViT qkv
    (1024, 1280, 1176, False, False, 0),    # patch embed (K not a multiple of 64)
    (1024, 5120, 1280, True, False, 1),     # fc1 + quick_gelu
    (1024, 1280, 5120, True, True, 0),      # fc2 + residual
    (256, 5120, 5120, True, False, 2),      # merger + gelu
    (275, 2048, 1536, True, False, 0),      # 2B prefill qkv (ragged M)
    (275, 17920, 1536, False, False, 0),    # 2B gate_up
    (275, 1536, 8960, False, True, 0),      # 2B down + residual
    (70, 512, 256, True, True, 3),          # tiny, silu
    (1, 36, 8, True, False, 0),             # degenerate
    (129, 132, 72, False, False, 0),        # ragged everything
    (275, 1536, 1536, False, True, 0),      # 2B o_proj + residual (split-K)
    (1024, 1280, 1280, True, True, 0),      # ViT proj (split-K 2)
    (64, 256, 4096, True, False, 1),        # deep split-K with activation
    (200, 128, 1000, False, False, 0),      # K not a multiple of 64 (register-staged kernel); K < 1024, so no split-K
    (70, 132, 1176, False, False, 0),       # K not a multiple of 64 AND split-K with a K tail (2 splits of 640)
    # shapes that take their (tile rows, split-K) from the tuned-plan table rather than from the cost model
    (290, 3584, 18944, False, True, 0),     # 7B down_proj (BM 128, 3 splits)
    (290, 4608, 3584, True, False, 0),      # 7B qkv (BM 64, 2 splits)
    (590, 3584, 18944, False, True, 0),     # 7B down_proj at two temporal grids per chunk (BM 128, 3 splits)
    (1024, 1280, 3424, True, True, 0),      # Qwen2.5 ViT down_proj (padded intermediate size)
    (256, 3584, 5120, True, False, 0),      # merger mlp.2 -> 7B
    (1024, 3840, 1280, True, False, 0),     # ViT qkv: 128-row tiles on 8 waves, one workgroup per CU
    (1000, 3840, 1280, True, False, 0),     # ... ragged in M
    # large M, long K: 128-row tiles on the 2-stage ring (the dense prefill's LLM passes), ragged in M and N
    (2100, 392, 2048, True, True, 0),
    (2048, 256, 2112, False, False, 1),
    (2048, 3584, 3584, True, True, 0),      # 224 tiles of 256 x 128 = one round at 87 %: the 8-wave tile is picked on its own
])
def test_gemm(ops, ref, M, N, K, bias, res, act):
    A, W = rnd((M, K), 1), rnd((N, K), 2, 0.05)
    b = rnd((N,), 3, 0.1) if bias else None
    r = rnd((M, N), 4) if res else None
    want = ref.gemm(A, W, b, r, act=act)
    got = ops.gemm(A.cuda(), W.cuda(), b.cuda() if bias else None, r.cuda() if res else None, act=act)
    close(f"gemm {M}x{N}x{K} act{act}", got, want)


@pytest.mark.parametrize("bm,splits", [(64, 1), (64, 5), (128, 1), (128, 3), (128, 8), (192, 1), (192, 4), (320, 1), (320, 8), (256, 1), (256, 4)])
def test_gemm_every_plan_is_numerically_the_same_op(diag, ref, bm, splits):
    """Tile height and split-K are performance choices only: forced through the tuning switches ON THE DIAGNOSTIC LIBRARY (the
    product library reads no environment), each plan must pass the same bar as the default one, and the library must report that it
    launched the forced plan.  tests/test_gemm_paths_gpu.py holds every plan to an fp64 per-element bound at ragged shapes."""
    import helpers as H
    import gemm_paths as G
    M, N, K = 290, 1536, 8960
    A, W, b, r_ = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((N,), 3, 0.1), rnd((M, N), 4)
    want = ref.gemm(A, W, bias=b, residual=r_)
    env = {"SVLM_GEMM_BM": bm, "SVLM_GEMM_SPLITS": splits}
    with H.forced_switches(env):
        got = diag.gemm(A.cuda(), W.cuda(), bias=b.cuda(), residual=r_.cuda())
        plan = diag.last_gemm_plan()
    exp = G.plan_bf16(M, N, K, env={k: str(v) for k, v in env.items()})
    assert plan["bm"] == bm and plan["splits"] == exp["splits"] and (splits == 1 or plan["splits"] >= 2), plan
    assert {k: plan[k] for k in ("bm", "waves", "stages", "dma", "splits", "kps", "table")} == {k: exp[k] for k in ("bm", "waves", "stages", "dma", "splits", "kps", "table")}
    close(f"gemm plan bm{bm} s{splits}", got, want)


@pytest.mark.parametrize("M,N,K", [(290, 1536, 8960), (290, 1536, 1536), (290, 3584, 18944), (33, 256, 512), (290, 17920, 1536)])
def test_gemm_norm_fused_reduce(ops, ref, M, N, K):
    """svlm_gemm_bf16_norm: residual-stream GEMM + the RMSNorm of its output rows (inside the split-K reduce when the plan
    splits K, a second launch otherwise, e.g. the (33, 256, 512) and the 17920-wide cases) == GEMM then RMSNorm, in place."""
    A, W, r_, g = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((M, N), 4), rnd((N,), 5, 0.1) + 1
    x_c, xn_c = r_.clone(), torch.empty((M, N), dtype=BF16)
    ref.gemm_norm(A, W, g, 1e-6, x_c, xn_c, residual=x_c)
    x_g, xn_g = r_.clone().cuda(), torch.empty((M, N), dtype=BF16, device="cuda")
    ops.gemm_norm(A.cuda(), W.cuda(), g.cuda(), 1e-6, x_g, xn_g, residual=x_g)
    close("gemm_norm out", x_g, x_c)
    close("gemm_norm norm", xn_g, xn_c, max_tol=2 ** -6)
    # against the norm kernel applied to the GPU's own GEMM output only the fp32 summation order of the mean square differs
    # (one workgroup per row here, one wave per row there): at most single bf16 roundings flip
    want = ops.rmsnorm(x_g, g.cuda(), 1e-6, out=torch.empty_like(x_g))
    d = (xn_g.float() - want.float()).abs()
    assert float(d.max()) <= 2 ** -7 * float(want.float().abs().max()) and float((d > 0).float().mean()) < 0.02


@pytest.mark.parametrize("M,I,K", [(290, 8960, 1536), (290, 18944, 3584), (590, 18944, 3584), (37, 104, 128), (130, 512, 256), (1, 64, 64), (2050, 192, 2048), (2048, 1792, 2048)])
def test_gemm_swiglu_epilogue(ops, diag, ref, M, I, K):
    """ACT_SWIGLU: W = [gate rows; up rows]; every tile pairs 64 gate with the 64 matching up columns and applies
    bf16(bf16(silu(g)) * u) in its epilogue == GEMM to (M, 2I) followed by svlm_silu_mul, for both tile heights."""
    A, W = rnd((M, K), 1), rnd((2 * I, K), 2, 0.05)
    want = ref.gemm(A, W, act=4)
    gu = ops.gemm(A.cuda(), W.cuda())
    sep = ops.silu_mul(gu, out=torch.empty((M, I), dtype=BF16, device="cuda"))
    import helpers as H
    for bm in (None, 64, 128):
        if bm is None:
            got = ops.gemm(A.cuda(), W.cuda(), act=4)
        else:                          # forced tile heights: on the diagnostic library, which must report the forced tile
            with H.forced_switches({"SVLM_GEMM_BM": bm}):
                got = diag.gemm(A.cuda(), W.cuda(), act=4)
                plan = diag.last_gemm_plan()
            assert plan["bm"] == (bm if M > 64 else 64) and plan["splits"] == 1, plan
        assert got.shape == (M, I)
        close(f"gemm swiglu bm={bm}", got, want)
        # (the large-M case's separate (M, 2I) GEMM has too few tiles and splits K: another summation order)
        assert torch.equal(got, sep) or bm is not None or M >= 2048, "default plan: same K order as the separate launches -> same bits"
    # with the [gate; up] bias of the Qwen2.5 vision MLP
    b = rnd((2 * I,), 3, 0.2)
    close("gemm swiglu + bias", ops.gemm(A.cuda(), W.cuda(), bias=b.cuda(), act=4), ref.gemm(A, W, bias=b, act=4))
    from streaming_vlm_amd._lib import SvlmError as _Err
    with pytest.raises(_Err):
        ops.gemm(A.cuda(), W.cuda(), residual=rnd((M, I), 4).cuda(), act=4)


@pytest.mark.parametrize("M,N,K", [(1024, 1280, 5120), (1024, 1280, 1280), (70, 160, 320)])
def test_gemm_layernorm_fused_reduce(ops, ref, M, N, K):
    """svlm_gemm_bf16_norm with a norm bias = LayerNorm (the ViT's proj -> norm2 and fc2 -> next norm1), fused into the split-K
    reduce for fc2's plan, a second launch for the others."""
    A, W, b, r_ = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((N,), 3, 0.1), rnd((M, N), 4)
    g, gb = rnd((N,), 5, 0.1) + 1, rnd((N,), 6, 0.1)
    x_c, xn_c = r_.clone(), torch.empty((M, N), dtype=BF16)
    ref.gemm_norm(A, W, g, 1e-6, x_c, xn_c, bias=b, residual=x_c, norm_b=gb)
    x_g, xn_g = r_.clone().cuda(), torch.empty((M, N), dtype=BF16, device="cuda")
    ops.gemm_norm(A.cuda(), W.cuda(), g.cuda(), 1e-6, x_g, xn_g, bias=b.cuda(), residual=x_g, norm_b=gb.cuda())
    close("gemm+LN out", x_g, x_c)
    want = ops.layernorm(x_g, g.cuda(), gb.cuda(), 1e-6, out=torch.empty_like(x_g))
    d = (xn_g.float() - want.float()).abs()
    assert float(d.max()) <= 2 ** -6 * float(want.float().abs().max()) and float((d > 0).float().mean()) < 0.02


def test_gemm_inplace_residual(ops, ref):
    A, W, x = rnd((300, 256), 1), rnd((512, 256), 2, 0.05), rnd((300, 512), 3)
    want = ref.gemm(A, W, None, x)
    xg = x.cuda()
    ops.gemm(A.cuda(), W.cuda(), residual=xg, out=xg)
    close("gemm in-place residual", xg, want)


def test_gemm_rejects_bad_shapes(ops):
    from streaming_vlm_amd._lib import SvlmError
    with pytest.raises(SvlmError):
        ops.gemm(rnd((4, 12), 1).cuda(), rnd((8, 12), 2).cuda())         # K % 8 != 0
    with pytest.raises(SvlmError):
        ops.gemm(rnd((4, 16), 1), rnd((8, 16), 2))                          # CPU tensors: no fallback


@pytest.mark.parametrize("N,K,bias,res,f32", [
    (2048, 1536, True, False, False), (1536, 1536, False, True, False), (17920, 1536, False, False, False),
    (1536, 8960, False, True, False), (151936, 1536, False, False, True), (520, 264, True, True, False), (7, 8, False, False, True),
    (3584, 18944, False, True, False), (100, 4104, True, False, False),
    # K-split path with a ragged last batch and odd N, a second batch per wave (K > 4 x 5 x 512), main path with K % 512 != 0
    (1535, 4104, True, True, False), (64, 12288, False, True, True), (4100, 1176, True, False, False), (16500, 520, False, True, False),
])
def test_gemv(ops, ref, N, K, bias, res, f32):
    x, W = rnd((K,), 1), rnd((N, K), 2, 0.05)
    b = rnd((N,), 3, 0.1) if bias else None
    r = rnd((N,), 4) if res else None
    want = ref.gemv(x, W, b, r, out=torch.empty(N, dtype=BF16))
    if f32:
        out = torch.empty(N, dtype=torch.float32, device="cuda")
        ops.gemv(x.cuda(), W.cuda(), b.cuda() if bias else None, r.cuda() if res else None, out_f32=out)
        assert torch.equal(out.cpu(), out.cpu().to(BF16).float()), "fp32 logits must be bf16-representable"
    else:
        out = ops.gemv(x.cuda(), W.cuda(), b.cuda() if bias else None, r.cuda() if res else None)
    close(f"gemv {N}x{K}", out, want)


# ----------------------------------------------------------------------------- norms / elementwise
@pytest.mark.parametrize("rows,cols", [(1, 1536), (275, 1536), (3, 3584), (5, 256), (1024, 1280)])
def test_rmsnorm_layernorm(ops, ref, rows, cols):
    x, w, b = rnd((rows, cols), 1, 3.0), rnd((cols,), 2) + 1, rnd((cols,), 3, 0.1)
    close("rmsnorm", ops.rmsnorm(x.cuda(), w.cuda(), 1e-6), ref.rmsnorm(x, w, 1e-6))
    close("layernorm", ops.layernorm(x.cuda(), w.cuda(), b.cuda(), 1e-6), ref.layernorm(x, w, b, 1e-6))


def test_add_silu_gather(ops, ref):
    a, b = rnd((33, 256), 1), rnd((33, 256), 2)
    close("add", ops.add(a.cuda(), b.cuda()), a + b, max_tol=0, mean_tol=0)
    gu = rnd((17, 1024), 3, 2.0)
    close("silu_mul", ops.silu_mul(gu.cuda()), ref.silu_mul(gu))
    table, alt = rnd((100, 64), 4), rnd((10, 64), 5)
    idx = torch.tensor([5, -1, 99, -10, 0, 7], dtype=torch.int32)
    out = torch.empty((6, 64), dtype=BF16, device="cuda")
    ops.gather_rows(table.cuda(), alt.cuda(), idx.cuda(), out)
    want = ref.gather_rows(table, alt, idx, torch.empty((6, 64), dtype=BF16))
    assert torch.equal(out.cpu(), want)
    off = torch.tensor([2], dtype=torch.int32, device="cuda")
    out1 = torch.empty((1, 64), dtype=BF16, device="cuda")
    ops.gather_rows(table.cuda(), None, idx.cuda(), out1, idx_off=off)
    assert torch.equal(out1.cpu()[0], table[99])


# ----------------------------------------------------------------------------- ViT attention
@pytest.mark.parametrize("n_seq,seq_len,H,d", [(1, 1024, 16, 80), (2, 256, 16, 80), (1, 64, 2, 80), (3, 16, 2, 80), (1, 100, 4, 128)])
def test_vit_rope_attn(ops, ref, n_seq, seq_len, H, d):
    N = n_seq * seq_len
    qkv = rnd((N, 3 * H * d), 1)
    ang = torch.rand((N, d // 2), generator=torch.Generator().manual_seed(2)) * 30
    cosT, sinT = ang.cos().contiguous(), ang.sin().contiguous()
    want_q = ref.vit_rope(qkv.clone(), cosT, sinT, H, d)
    got_q = ops.vit_rope(qkv.cuda(), cosT.cuda(), sinT.cuda(), H, d)
    close("vit_rope", got_q, want_q)
    scale = 1 / math.sqrt(d)
    # feed BOTH attention implementations the same rotated buffer
    want = ref.vit_attn(want_q, n_seq, seq_len, H, d, scale)
    got = ops.vit_attn(want_q.cuda(), n_seq, seq_len, H, d, scale)
    close(f"vit_attn {n_seq}x{seq_len} H{H} d{d}", got, want, max_tol=2 ** -6, mean_tol=1e-3)


# ----------------------------------------------------------------------------- rope table / KV pool
def test_mrope_table(ops, ref):
    L, D = 300, 128
    g = torch.Generator().manual_seed(0)
    pos3 = torch.randint(0, 5000, (3, 512), generator=g, dtype=torch.int32)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    want = torch.zeros((512, D), dtype=BF16)
    ref.mrope_table(pos3, inv, want, 7, L, [16, 24, 24])
    got = torch.zeros((512, D), dtype=BF16, device="cuda")
    ops.mrope_table(pos3.cuda(), inv.cuda(), got, 7, L, [16, 24, 24])
    diff = (got.cpu().float() - want.float()).abs()
    print(f"[mrope_table] max diff {float(diff.max()):.3e} mismatched {float((diff > 0).float().mean()):.5f}")
    assert float(diff.max()) <= 2 ** -7        # one bf16 ulp at |x|<=1 (libm vs ocml last-bit differences)
    assert float((diff > 0).float().mean()) < 0.02
    assert torch.equal(got.cpu()[:7], torch.zeros((7, D), dtype=BF16))    # rows outside [start, start+count) untouched


def _pool(layers=2, Hkv=2, n_slots=96, D=128, seed=0):
    return rnd((layers, 2, Hkv, n_slots, D), seed)


def test_kv_append_gather_move(ops, ref):
    pool_c = _pool()
    pool_g = pool_c.clone().cuda()
    Hkv, D, n_slots = 2, 128, 96
    perm = torch.randperm(n_slots, generator=torch.Generator().manual_seed(1)).to(torch.int32)
    slot_of = perm[:64].clone()
    T = 9
    qkv = rnd((T, 3 * Hkv * D), 2)
    k_new, v_new = qkv[:, Hkv * D:2 * Hkv * D], qkv[:, 2 * Hkv * D:]
    qkv_g = qkv.cuda()
    ref.kv_append(k_new, v_new, pool_c, 1, slot_of, 20, T)
    ops.kv_append(qkv_g[:, Hkv * D:2 * Hkv * D], qkv_g[:, 2 * Hkv * D:], pool_g, 1, slot_of.cuda(), 20, T)
    assert torch.equal(pool_g.cpu(), pool_c), "kv_append (host start)"
    len_dev = torch.tensor([31], dtype=torch.int32, device="cuda")
    ref.kv_append(k_new[:1], v_new[:1], pool_c, 0, slot_of, 31, 1)
    ops.kv_append(qkv_g[:1, Hkv * D:2 * Hkv * D], qkv_g[:1, 2 * Hkv * D:], pool_g, 0, slot_of.cuda(), 0, 1, len_dev=len_dev)
    assert torch.equal(pool_g.cpu(), pool_c), "kv_append (device length)"
    for which in (0, 1):
        assert torch.equal(ops.kv_gather(pool_g, 1, which, slot_of.cuda(), 40).cpu(), ref.kv_gather(pool_c, 1, which, slot_of, 40))
    src, dst = perm[:10].clone(), perm[64:74].clone()
    ref.kv_move_rows(pool_c, src, dst)
    ops.kv_move_rows(pool_g, src.cuda(), dst.cuda())
    assert torch.equal(pool_g.cpu(), pool_c), "kv_move_rows"


# ----------------------------------------------------------------------------- LLM attention
def _attn_setup(Hq, Hkv, L, cap, seed):
    D = 128
    n_slots = cap + 32
    pool = rnd((1, 2, Hkv, n_slots, D), seed)
    perm = torch.randperm(n_slots, generator=torch.Generator().manual_seed(seed + 1)).to(torch.int32)
    slot_of = perm[:cap].clone().contiguous()
    pos3 = torch.randint(0, 3000, (3, cap), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.int32)
    inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))
    rope = torch.zeros((cap, D), dtype=BF16)
    from ref_ops import RefOps
    RefOps().mrope_table(pos3, inv, rope, 0, cap, [16, 24, 24])
    return pool, slot_of, rope


@pytest.mark.parametrize("Hq,Hkv,L,chunk", [(12, 2, 2352, 64), (12, 2, 2352, 32), (28, 4, 4400, 64), (4, 2, 1, 16), (4, 2, 17, 16),
                                            (12, 2, 100, 32), (8, 1, 333, 48), (12, 2, 2052, 16), (3, 1, 70, 64), (10, 2, 130, 64),
                                            # multi-pass (long-cache) kernel: full / ragged last pass, one pass only, odd pass counts, G=7
                                            (12, 2, 9000, 256), (12, 2, 300, 128), (28, 4, 4400, 128), (4, 2, 65, 128), (8, 1, 1000, 512),
                                            (4, 2, 3, 128), (12, 2, 2352, 192), (6, 1, 8191, 512)])
def test_decode_attn(ops, ref, Hq, Hkv, L, chunk):
    cap = ((L + 63) // 64) * 64 + 64
    pool, slot_of, rope = _attn_setup(Hq, Hkv, L, cap, 10)
    q = rnd((Hq * 128,), 3)
    scale = 1 / math.sqrt(128)
    want = ref.decode_attn(q, pool, 0, slot_of, rope, torch.empty(Hq * 128, dtype=BF16), None, Hq, cap, chunk, scale, length=L)
    ws = ops.decode_attn_ws(Hq, cap, chunk, "cuda")
    out = torch.empty(Hq * 128, dtype=BF16, device="cuda")
    pg, sg, rg = pool.cuda(), slot_of.cuda(), rope.cuda()
    ops.decode_attn(q.cuda(), pg, 0, sg, rg, out, ws, Hq, cap, chunk, scale, length=L)
    close(f"decode_attn Hq{Hq} Hkv{Hkv} L{L} chunk{chunk}", out, want, max_tol=2 ** -6, mean_tol=1e-3)
    # device-resident length (graph replay path): *len_dev + 1
    len_dev = torch.tensor([L - 1], dtype=torch.int32, device="cuda")
    out2 = torch.empty_like(out)
    ops.decode_attn(q.cuda(), pg, 0, sg, rg, out2, ws, Hq, cap, chunk, scale, length=1, len_dev=len_dev)
    assert torch.equal(out2, out)
    # rows the sequence does not map to may hold anything (a pool need not be zero-filled, pages are recycled): NaN in every slot
    # outside slot_of[:L] must not reach the output (0 x NaN inside the P.V MFMA of a tile that crosses the end of the cache)
    used = torch.zeros(pool.shape[3], dtype=torch.bool)
    used[slot_of[:L].long()] = True
    pn = pool.clone()
    pn[:, :, :, ~used] = float("nan")
    out3 = torch.empty_like(out)
    ops.decode_attn(q.cuda(), pn.cuda(), 0, sg, rg, out3, ws, Hq, cap, chunk, scale, length=L)
    assert torch.equal(out3, out), "stale / non-finite pool rows behind the end of the sequence leak into the output"


@pytest.mark.parametrize("Hq,Hkv,L,chunk,T", [(12, 2, 2352, 48, 275), (12, 2, 2352, 64, 1), (28, 4, 4400, 48, 300), (4, 2, 40, 16, 40), (8, 1, 333, 48, 17),
                                              # streaming kernel: the tile that holds the boundary, boundaries on / off a tile edge, G = 7
                                              (12, 2, 9000, 256, 500), (28, 4, 4400, 128, 4400), (12, 2, 2352, 192, 100), (6, 1, 8191, 512, 31),
                                              (4, 2, 300, 128, 300)])
def test_decode_attn_from_the_linear_planes_the_prefill_leaves(ops, ref, Hq, Hkv, L, chunk, T):
    """svlm_prefill_attn_ropeload_lin leaves rotated keys (tile layout of include/svlm.h) + values of rows [0, L) and lin_state = {L, 1};
    svlm_dec_qkv_lin adds every appended row (key un-rotated); svlm_decode_attn_lin must give the SAME BITS as the pool path for every
    later length, every validity bound, with and without the appended rows in the planes."""
    from ref_ops import RefOps
    new = 24                                       # rows appended after the prefill (decode steps)
    cap = ((L + new + 63) // 64) * 64 + 64
    pool, slot_of, rope = _attn_setup(Hq, Hkv, L, cap, 30)
    scale = 1 / math.sqrt(128)
    pg, sg, rg = pool.cuda(), slot_of.cuda(), rope.cuda()
    lin_rows = -(-cap // 16) * 16
    planes = torch.full((1, 2, Hkv, lin_rows, 128), float("nan"), dtype=BF16, device="cuda")      # never read above the rows written
    lin_state = torch.zeros(2, dtype=torch.int32, device="cuda")
    qp = rnd((T, Hq * 128), 6).cuda()
    out_p, out_p2 = torch.empty((T, Hq * 128), dtype=BF16, device="cuda"), torch.empty((T, Hq * 128), dtype=BF16, device="cuda")
    ops.prefill_attn(qp, pg, 0, sg, rg, out_p, T, L, Hq, scale)
    ops.prefill_attn(qp, pg, 0, sg, rg, out_p2, T, L, Hq, scale, lin=(planes, lin_state))
    assert torch.equal(out_p, out_p2) and lin_state.tolist() == [L, 1]
    Kr = ref._rot(pool[0, 0][:, slot_of[:L].long()], rope, torch.arange(L))
    assert torch.equal(RefOps.lin_k_rows(planes[0, 0].cpu(), L), Kr), "rotated keys in the linear planes"
    assert torch.equal(planes[0, 1][:, :L].cpu(), pool[0, 1][:, slot_of[:L].long()]), "values in the linear planes"
    # ---- decode steps append rows L .. L + new - 1 through the QKV launch: pool slot AND linear planes
    qd, kd, Kx = Hq * 128, Hkv * 128, 256
    W, bias, lnw = rnd((qd + 2 * kd, Kx), 7, 0.08).cuda(), rnd((qd + 2 * kd,), 8).cuda(), (rnd((Kx,), 9) + 1).cuda()
    q_out = torch.empty(qd, dtype=BF16, device="cuda")
    len_dev = torch.zeros(1, dtype=torch.int32, device="cuda")
    for r in range(L, L + new):
        x = rnd((Kx,), 100 + r).cuda()
        if r % 2:
            ops.dec_qkv(x, lnw, 1e-6, W, bias, q_out, pg, 0, sg, qd, kd, length=r, lin=(planes, lin_state))
        else:
            len_dev.fill_(r)
            ops.dec_qkv(x, lnw, 1e-6, W, bias, q_out, pg, 0, sg, qd, kd, len_dev=len_dev, lin=(planes, lin_state))
    rows_new = slot_of[L:L + new].long()
    pool2 = pg.cpu()
    assert torch.equal(RefOps.lin_k_rows(planes[0, 0].cpu(), L + new)[:, L:], pool2[0, 0][:, rows_new]), "appended keys (un-rotated) in the linear planes"
    assert torch.equal(planes[0, 1][:, L:L + new].cpu(), pool2[0, 1][:, rows_new]), "appended values in the linear planes"
    assert torch.equal(RefOps.lin_k_rows(planes[0, 0].cpu(), L), Kr), "the appends left the rotated rows alone"
    ws = ops.decode_attn_ws(Hq, cap, chunk, "cuda")
    q = rnd((Hq * 128,), 3).cuda()
    for Ld in (L, L + 1, L + 7, L + new):          # the prefill's own length, the first decode step, one in the middle, the last one
        want = torch.empty(Hq * 128, dtype=BF16, device="cuda")
        ops.decode_attn(q, pg, 0, sg, rg, want, ws, Hq, cap, chunk, scale, length=Ld)
        for valid in sorted({L, max(L - 1, 0), L // 2, (L // 16) * 16, min(L, 15), 0}):
            for fresh in (1, 0):
                if fresh and valid != L:
                    continue                    # appended rows follow a bound the prefill set; a lowered bound always clears the flag
                lin_state.copy_(torch.tensor([valid, fresh], dtype=torch.int32))
                got = torch.full_like(want, float("nan"))
                ops.decode_attn(q, pg, 0, sg, rg, got, ws, Hq, cap, chunk, scale, length=Ld, lin=(planes, lin_state))
                assert torch.equal(got, want), f"L={Ld} lin_state=({valid}, {fresh}): linear planes and pool path differ"
                len_dev.fill_(Ld - 1)
                got2 = torch.full_like(want, float("nan"))
                ops.decode_attn(q, pg, 0, sg, rg, got2, ws, Hq, cap, chunk, scale, length=1, len_dev=len_dev, lin=(planes, lin_state))
                assert torch.equal(got2, want), f"L={Ld} lin_state=({valid}, {fresh}) (device length)"
    # a bound ABOVE the cache length (a host that truncated without lowering it) is clamped, not trusted
    Ls = max(L - 20, 1)
    want = torch.empty(Hq * 128, dtype=BF16, device="cuda")
    ops.decode_attn(q, pg, 0, sg, rg, want, ws, Hq, cap, chunk, scale, length=Ls)
    for fresh in (0, 1):
        lin_state.copy_(torch.tensor([L, fresh], dtype=torch.int32))
        got = torch.empty_like(want)
        ops.decode_attn(q, pg, 0, sg, rg, got, ws, Hq, cap, chunk, scale, length=Ls, lin=(planes, lin_state))
        assert torch.equal(got, want)


# (2,1,700,700) and (4,2,300,1000) run 5 / 7 key splits whose last ones start beyond some queries' causal limit (rows that
# are fully masked inside a split); (12,2,275,2330) is the steady-state chunk of BASELINE configs[1] (4 splits)
@pytest.mark.parametrize("Hq,Hkv,T,L", [(12, 2, 275, 2330), (28, 4, 40, 300), (4, 2, 1, 1), (4, 2, 20, 20), (4, 2, 37, 100), (6, 1, 16, 48),
                                        (2, 1, 700, 700), (4, 2, 300, 1000), (2, 2, 130, 257),
                                        # T >= 1024 without key splits: two query blocks per wave (the dense prefill's 4096-row passes)
                                        (4, 2, 1100, 1500), (7, 1, 1024, 1024), (2, 1, 1090, 3001)])
def test_prefill_attn(ops, ref, Hq, Hkv, T, L):
    cap = ((L + 63) // 64) * 64
    pool, slot_of, rope = _attn_setup(Hq, Hkv, L, cap, 20)
    q = rnd((T, Hq * 128), 5)
    scale = 1 / math.sqrt(128)
    want = ref.prefill_attn(q, pool, 0, slot_of, rope, torch.empty((T, Hq * 128), dtype=BF16), T, L, Hq, scale)
    out = torch.empty((T, Hq * 128), dtype=BF16, device="cuda")
    ops.prefill_attn(q.cuda(), pool.cuda(), 0, slot_of.cuda(), rope.cuda(), out, T, L, Hq, scale)
    close(f"prefill_attn Hq{Hq} Hkv{Hkv} T{T} L{L}", out, want, max_tol=2 ** -6, mean_tol=1e-3)


@pytest.mark.parametrize("T,L,step", [(1100, 1500, False), (200, 900, False), (64, 64, False), (1100, 1500, True), (300, 640, True)])
def test_prefill_attn_reference_moves_along_the_sequence(ops, ref, T, L, step):
    """The prefill kernel keeps a LAZY softmax reference (exact maximum only when a lane's partial row sum leaves the safe range).
    Keys whose scores climb by ~160 binades along the sequence (or jump by ~300 at once) force the reference to move again and again, the first jumps past
    the range of exp2 itself (+inf in the fast path, which must be caught before it is used)."""
    Hq, Hkv = 2, 1
    cap = ((L + 63) // 64) * 64
    pool, slot_of, _ = _attn_setup(Hq, Hkv, L, cap, 33)
    rope = torch.zeros((cap, 128), dtype=BF16)
    rope[:, :64] = 1.0                                      # cos = 1, sin = 0: no rotation
    u = torch.full((128,), 0.5)
    ramp = torch.arange(L, dtype=torch.float32) * (40.0 / L)
    if step:                                                # ... or jump by ~300 binades in the middle of a tile, half way through
        ramp = torch.where(torch.arange(L) < L - T // 2 - 5, torch.zeros(L), torch.full((L,), 75.0))
    k_rows = (u[None, :] * ramp[:, None]).to(BF16)          # q.k * scale * log2(e) runs from 0 to ~163
    pool[0, 0, 0, slot_of[:L].long()] = k_rows
    q = (u.repeat(Hq)[None, :] + rnd((T, Hq * 128), 7, 0.01).float()).to(BF16).contiguous()
    scale = 1 / math.sqrt(128)
    want = ref.prefill_attn(q, pool, 0, slot_of, rope, torch.empty((T, Hq * 128), dtype=BF16), T, L, Hq, scale)
    out = torch.empty((T, Hq * 128), dtype=BF16, device="cuda")
    ops.prefill_attn(q.cuda(), pool.cuda(), 0, slot_of.cuda(), rope.cuda(), out, T, L, Hq, scale)
    assert torch.isfinite(out.float()).all()
    close(f"prefill_attn climbing scores T{T} L{L}", out, want, max_tol=2 ** -6, mean_tol=1e-3)


def test_prefill_attn_appends_the_new_rows(ops, ref):
    """k_new / v_new handed to the prefill attention are written to their pool slots (== svlm_kv_append) by the launch that
    rotates the keys, and the result equals append-then-attend."""
    Hq, Hkv, T, L = 12, 2, 70, 333
    cap = 384
    pool, slot_of, rope = _attn_setup(Hq, Hkv, L, cap, 21)
    q, kn, vn = rnd((T, Hq * 128), 5), rnd((T, Hkv * 128), 6), rnd((T, Hkv * 128), 7)
    scale = 1 / math.sqrt(128)
    pool_c = pool.clone()
    want = ref.prefill_attn(q, pool_c, 0, slot_of, rope, torch.empty((T, Hq * 128), dtype=BF16), T, L, Hq, scale, k_new=kn, v_new=vn)
    # hand the rows over as column slices of one fused buffer, like the engine does
    fused = torch.cat([q, kn, vn], 1).cuda()
    pool_g = pool.clone().cuda()
    out = torch.empty((T, Hq * 128), dtype=BF16, device="cuda")
    ops.prefill_attn(fused[:, :Hq * 128], pool_g, 0, slot_of.cuda(), rope.cuda(), out, T, L, Hq, scale,
                     k_new=fused[:, Hq * 128:(Hq + Hkv) * 128], v_new=fused[:, (Hq + Hkv) * 128:])
    close("prefill_attn with append", out, want, max_tol=2 ** -6, mean_tol=1e-3)
    assert torch.equal(pool_g.cpu(), pool_c), "pool rows after the fused append differ from svlm_kv_append semantics"


def test_prefill_matches_decode_on_last_row(ops):
    """Size-independent property: the last prefill row equals a decode step over the same cache."""
    Hq, Hkv, T, L = 12, 2, 64, 1500
    cap = 1536
    pool, slot_of, rope = _attn_setup(Hq, Hkv, L, cap, 30)
    q = rnd((T, Hq * 128), 6).cuda()
    scale = 1 / math.sqrt(128)
    out = torch.empty((T, Hq * 128), dtype=BF16, device="cuda")
    pg, sg, rg = pool.cuda(), slot_of.cuda(), rope.cuda()
    ops.prefill_attn(q, pg, 0, sg, rg, out, T, L, Hq, scale)
    ws = ops.decode_attn_ws(Hq, cap, 64, "cuda")
    o1 = torch.empty(Hq * 128, dtype=BF16, device="cuda")
    ops.decode_attn(q[T - 1].contiguous(), pg, 0, sg, rg, o1, ws, Hq, cap, 64, scale, length=L)
    close("prefill last row vs decode", out[T - 1], o1, max_tol=2 ** -6, mean_tol=1e-3)


def test_kvpool_reference_cache_contract_on_device(ops):
    """update() / key_cache[i] = ... / iteration of the reference's cache object, through svlm_kv_append / svlm_kv_gather."""
    import streaming_vlm_amd as S
    pool = S.KVPool(3, 2, 128, 256, "cuda", ops, page_tokens=16, slack=0.25)
    ref = [[None, None] for _ in range(3)]
    for j, T in enumerate((50, 1, 7)):
        for layer in range(3):
            k, v = rnd((1, 2, T, 128), 40 + 10 * j + layer).cuda(), rnd((1, 2, T, 128), 80 + 10 * j + layer).cuda()
            ref[layer][0] = k if ref[layer][0] is None else torch.cat([ref[layer][0], k], 2)
            ref[layer][1] = v if ref[layer][1] is None else torch.cat([ref[layer][1], v], 2)
            ko, vo = pool.update(k, v, layer, None)
            assert torch.equal(ko, ref[layer][0]) and torch.equal(vo, ref[layer][1])
    keep = torch.tensor([i for i in range(58) if not 4 <= i <= 30], device="cuda")
    for i, (k, v) in enumerate(list(pool)):
        pool.key_cache[i] = torch.index_select(k, 2, keep)
        pool.value_cache[i] = torch.index_select(v, 2, keep)
    assert pool.get_seq_length() == 31
    other = S.KVPool(3, 2, 128, 256, "cuda", ops, page_tokens=16, slack=0.25)
    for layer in range(3):
        other.update(ref[layer][0], ref[layer][1], layer)
    other.prune(4, 30)
    for layer, ((k0, v0), (k1, v1)) in enumerate(zip(pool, other)):
        assert torch.equal(k0, k1) and torch.equal(v0, v1)
        assert torch.equal(k0, ref[layer][0][:, :, keep]) and torch.equal(v0, ref[layer][1][:, :, keep])


@pytest.mark.parametrize("T,H,W", [(1, 448, 448), (2, 448, 448), (3, 56, 84), (1, 224, 224), (4, 28, 28)])
def test_patchify_u8_bit_exact(ops, T, H, W):
    """GPU frame ingest == the host processor's rescale / normalise / merge-block-major patchify, bit for bit in bf16
    (odd T: the last frame is repeated to fill its temporal patch)."""
    from streaming_vlm_amd.synthetic import patchify
    g = torch.Generator().manual_seed(T * 1000 + H + W)
    frames = torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8)
    want, grid_w = patchify(frames)
    got, grid = ops.patchify_u8(frames.cuda())
    assert grid == grid_w and got.shape == want.shape
    assert torch.equal(got.cpu(), want.to(BF16))
    with pytest.raises(Exception):
        ops.patchify_u8(torch.zeros((1, 3, 30, 28), dtype=torch.uint8, device="cuda"))


# ----------------------------------------------------------------------------- sampling
def test_penalty_argmax(ops, ref):
    V = 151936
    g = torch.Generator().manual_seed(0)
    logits = torch.randn(V, generator=g)
    logits = logits.to(BF16).float()
    ids = torch.randint(0, V, (500,), generator=g, dtype=torch.int32)
    top = int(torch.argmax(logits))
    ids[0] = top                                    # the raw winner is penalised
    sws = ops.sampling_ws(V, "cuda")
    for suppress in (None, torch.tensor([151645, 151643], dtype=torch.int32)):
        seen_c = torch.zeros(V, dtype=torch.uint8)
        ref.mark_seen(ids, 500, seen_c)
        seen_g = torch.zeros(V, dtype=torch.uint8, device="cuda")
        ops.mark_seen(ids.cuda(), 500, seen_g)
        assert torch.equal(seen_g.cpu(), seen_c)
        tb_c, st_c = torch.zeros(8, dtype=torch.int32), torch.tensor([100, -1], dtype=torch.int32)
        tb_g, st_g = tb_c.clone().cuda(), st_c.clone().cuda()
        lg = logits.clone()
        if suppress is not None:
            lg[151645] = 100.0
        for adv in (0, 1, 1):
            ref.penalty_argmax(lg, seen_c, 1.05, suppress, tb_c, st_c, adv)
            ops.penalty_argmax(lg.cuda(), seen_g, 1.05, suppress.cuda() if suppress is not None else None, tb_g, st_g, adv, sws)
        assert torch.equal(tb_g.cpu(), tb_c) and torch.equal(st_g.cpu(), st_c) and torch.equal(seen_g.cpu(), seen_c)
    # ties resolve to the lowest index like torch.argmax
    flat = torch.zeros(V)
    tb, st = torch.zeros(4, dtype=torch.int32, device="cuda"), torch.tensor([0, -1], dtype=torch.int32, device="cuda")
    ops.penalty_argmax(flat.cuda(), None, 1.0, None, tb, st, 0, sws)
    assert int(tb[0]) == 0


# ----------------------------------------------------------------------------- fused decode-step kernels
# hidden sizes pick the (pre-issued K-steps, x chunks per thread) variant: <=1536 (3,1), <=2048 (4,1), <=4096 (4,2), else (4,4)
@pytest.mark.parametrize("H,Hq,Hkv,I,V", [(1536, 12, 2, 8960, 151936), (3584, 28, 4, 18944, 152064), (256, 4, 2, 512, 151680),
                                          (2048, 16, 2, 1000, 5000), (8192, 8, 8, 520, 3001), (1544, 4, 2, 36, 130)])
def test_fused_decode_kernels(ops, ref, H, Hq, Hkv, I, V):
    D = 128
    qd, kd = Hq * D, Hkv * D
    x, lnw = rnd((H,), 1, 2.0), rnd((H,), 2, 0.1) + 1
    # --- norm + qkv + append
    W, b = rnd((qd + 2 * kd, H), 3, 0.03), rnd((qd + 2 * kd,), 4, 0.1)
    pool_c = rnd((2, 2, Hkv, 48, D), 5)
    pool_g = pool_c.clone().cuda()
    slot_of = torch.randperm(48, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    q_c, q_g = torch.zeros(qd + 2 * kd, dtype=BF16), torch.zeros(qd + 2 * kd, dtype=BF16, device="cuda")
    ref.dec_qkv(x, lnw, 1e-6, W, b, q_c, pool_c, 1, slot_of, qd, kd, length=17)
    len_dev = torch.tensor([17], dtype=torch.int32, device="cuda")
    ops.dec_qkv(x.cuda(), lnw.cuda(), 1e-6, W.cuda(), b.cuda(), q_g, pool_g, 1, slot_of.cuda(), qd, kd, len_dev=len_dev)
    close("dec_qkv q", q_g[:qd], q_c[:qd])
    close("dec_qkv pool", pool_g, pool_c)
    assert torch.equal(pool_g.cpu()[0], pool_c[0]), "other layers untouched"
    # --- norm + gate/up + swiglu
    Wgu = rnd((2 * I, H), 7, 0.03)
    h_c, h_g = torch.zeros(I, dtype=BF16), torch.zeros(I, dtype=BF16, device="cuda")
    ref.dec_gate_up(x, lnw, 1e-6, Wgu, h_c)
    ops.dec_gate_up(x.cuda(), lnw.cuda(), 1e-6, Wgu.cuda(), h_g)
    close("dec_gate_up", h_g, h_c)
    # --- final norm + lm_head + penalty + argmax + feedback
    Wl = rnd((V, H), 8, 0.03)
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (300,), generator=g, dtype=torch.int32)
    sup = torch.tensor([151645, 151643] if V > 151645 else [V - 7, V - 3], dtype=torch.int32)
    lg_c, lg_g = torch.zeros(V), torch.zeros(V, device="cuda")
    seen_c = torch.zeros(V, dtype=torch.uint8)
    ref.mark_seen(ids, 300, seen_c)
    seen_g = seen_c.clone().cuda()
    sws = ops.sampling_ws(V, "cuda")
    tb_c, st_c = torch.zeros(4, dtype=torch.int32), torch.tensor([50, 0], dtype=torch.int32)
    tb_g, st_g = tb_c.clone().cuda(), st_c.clone().cuda()
    ref.dec_lm_head(x, lnw, 1e-6, Wl, lg_c, seen_c, 1.05, sup, None)
    ref.argmax_finish(None, V, seen_c, tb_c, st_c, 1)
    ops.dec_lm_head(x.cuda(), lnw.cuda(), 1e-6, Wl.cuda(), lg_g, seen_g, 1.05, sup.cuda(), sws)
    ops.argmax_finish(sws, V, seen_g, tb_g, st_g, 1)
    close("dec_lm_head logits", lg_g, lg_c)
    # the fused argmax must agree with a host argmax over the GPU's own logits (exact), and with the oracle
    sc = lg_g.cpu().clone()
    m = seen_c.bool().clone(); m[int(tb_c[1])] = seen_c[int(tb_c[1])].bool()
    seen0 = torch.zeros(V, dtype=torch.uint8); ref.mark_seen(ids, 300, seen0)
    mm = seen0.bool()
    sc[mm] = torch.where(sc[mm] < 0, sc[mm] * 1.05, sc[mm] / 1.05)
    sc[sup.long()] = float("-inf")
    assert int(tb_g[1]) == int(torch.argmax(sc)), "fused argmax != argmax of its own logits"
    assert torch.equal(st_g.cpu(), st_c)
    if int(tb_g[1]) != int(tb_c[1]):
        print("[fused] token differs from oracle (top-2 margin inside rounding noise)")


# ----------------------------------------------------------------------------- frame resize
@pytest.mark.parametrize("T,H,W,h,w", [(2, 360, 640, 252, 448), (1, 240, 320, 336, 448), (3, 100, 80, 56, 42), (2, 64, 64, 64, 64),
                                       (1, 37, 53, 28, 28), (2, 720, 1280, 252, 448), (1, 30, 40, 56, 70), (1, 1080, 1920, 560, 1008)])
def test_resize_bicubic_aa_u8_bit_exact(ops, T, H, W, h, w):
    """svlm_resize_bicubic_aa_u8 == the oracle's restatement of torch's CPU antialias kernel, bit for bit (down- and up-scaling, 5
    to 13 taps per axis, identity at equal sizes) == torch.nn.functional.interpolate itself; the oracle is pinned to torch's fp32 bits
    in tests/test_resize.py."""
    from oracle import resize as R
    g = torch.Generator().manual_seed(H * 3 + w + T)
    x = torch.randint(0, 256, (T, 3, H, W), generator=g, dtype=torch.uint8)
    if T > 1:
        x[1] = (torch.arange(W).view(1, 1, W) * 255 // (W - 1) + torch.arange(H).view(1, H, 1)).clamp(0, 255).to(torch.uint8)
    want = R.resize_bicubic_aa_u8(x.numpy(), h, w)
    got = ops.resize_u8(x.cuda(), h, w)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (T, 3, h, w)
    assert np.array_equal(got.cpu().numpy(), want)
    again = ops.resize_u8(x.cuda(), h, w)                 # cached tables, reused scratch
    assert torch.equal(again, got)
    # and against the reference's own call on this box: torch's CPU antialias kernel in float32, clamp, round, cast (torchvision v1 resize)
    ref = torch.nn.functional.interpolate(x.float(), size=(h, w), mode="bicubic", antialias=True, align_corners=False).clamp(0, 255).round().to(torch.uint8)
    assert torch.equal(got.cpu(), ref), f"{int((got.cpu() != ref).sum())} pixels differ from torch's interpolate"
    with pytest.raises(Exception):
        ops.resize_u8(x.cuda().float(), h, w)


# ----------------------------------------------------------------------------- device-side sampling
def _chi2_p(counts, probs, n):
    """p-value of the observed token counts against `probs`; cells pooled until each expects >= 25 draws."""
    from scipy import stats
    order = np.argsort(-probs)
    obs, exp, o_acc, e_acc = [], [], 0.0, 0.0
    for i in order:
        o_acc += counts[i]; e_acc += probs[i] * n
        if e_acc >= 25:
            obs.append(o_acc); exp.append(e_acc); o_acc = e_acc = 0.0
    if e_acc > 0 and obs:
        obs[-1] += o_acc; exp[-1] += e_acc
    exp = np.array(exp) * (np.sum(obs) / np.sum(exp))
    return float(stats.chisquare(obs, exp).pvalue), len(obs)


@pytest.mark.parametrize("V,temperature,top_k,top_p,penalty", [
    (5000, 0.9, 0, 1.0, 1.05),       # the reference's call: T = 0.9, repetition penalty 1.05 -- Gumbel-max in the argmax kernels
    (5000, 0.7, 40, 1.0, 1.0),       # top-k
    (5000, 1.0, 0, 0.8, 1.0),        # nucleus only (survivors beyond 2048 are cut: the nucleus here is far smaller)
    (5000, 0.9, 50, 0.9, 1.05),      # HF defaults-style mix
    (151936, 0.9, 0, 1.0, 1.05),     # full vocabulary
    (151936, 0.9, 0, 0.95, 1.05),    # full vocabulary, nucleus weighed against all of it
])
def test_penalty_sample_distribution(ops, V, temperature, top_k, top_p, penalty):
    """svlm_penalty_sample against the oracle's restatement of HF's processors (oracle/generate.py:warp_scores + softmax):
    1e5 draws from fixed logits, chi-square over pooled cells (p > 1e-4); every draw must fall inside the survivor set."""
    from oracle import generate as og
    N = 100_000
    g = torch.Generator().manual_seed(V + top_k)
    logits = (torch.randn(V, generator=g) * 2.0)
    seen_ids = torch.randint(0, V, (64,), generator=g)
    sup = torch.tensor([7, 11], dtype=torch.int32)
    sc = og.repetition_penalty(logits.clone(), seen_ids.tolist(), penalty)
    sc[sup.long()] = float("-inf")
    probs = torch.softmax(og.warp_scores(sc, temperature, top_k, top_p), dim=-1).double().numpy()
    seen = torch.zeros(V, dtype=torch.uint8)
    seen[seen_ids] = 1
    d_logits, d_seen, d_sup = logits.cuda(), seen.cuda(), sup.cuda()
    tok_buf = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    state = torch.tensor([0, -1], dtype=torch.int32, device="cuda")
    rng = torch.tensor([12345, 678], dtype=torch.int32, device="cuda")
    ws = ops.sampling_ws(V, "cuda")
    seen_arg = d_seen if penalty != 1.0 else None
    seen0 = seen.cuda()
    for _ in range(N):
        ops.penalty_sample(d_logits, seen_arg, penalty, d_sup, temperature, top_k, top_p, rng, tok_buf, state, 0, ws)
        if seen_arg is not None:
            d_seen.copy_(seen0)          # the kernel marks the token it drew: every draw must see the same `seen` set
    torch.cuda.synchronize()
    toks = tok_buf[:N].cpu().numpy()
    assert int(state[1]) == N - 1
    counts = np.bincount(toks, minlength=V).astype(np.float64)
    assert counts[probs == 0].sum() == 0, "a draw fell outside the survivor set"
    p, cells = _chi2_p(counts, probs, N)
    print(f"[sample V={V} T={temperature} k={top_k} p={top_p}] {cells} cells, chi-square p = {p:.3g}, support {int((probs > 0).sum())}")
    assert p > 1e-4, p


def test_penalty_sample_multi_level_radix_descent(ops):
    """top-k over 20000 scores that all fall into ONE 11-bit radix bin (same exponent, same two leading mantissa bits): the candidate
    range has to be narrowed by the second and third level of the descent.  Every thread must use the same `above` count at each level
    (a workgroup barrier separates its read from the finder's update): a thread that saw the updated count would pick a higher bin, the
    list would hold fewer than k candidates and the draw would come from a truncated top-k set -- caught here by the distribution
    test over the oracle's top-k survivors."""
    from oracle import generate as og
    V, N, top_k, T = 20000, 60_000, 50, 0.9
    g = torch.Generator().manual_seed(77)
    logits = 8.0 + torch.rand(V, generator=g) * 0.99                 # [8, 8.99): one quarter-octave
    probs = torch.softmax(og.warp_scores(logits.clone(), T, top_k, 1.0), dim=-1).double().numpy()
    assert int((probs > 0).sum()) == top_k
    d_logits = logits.cuda()
    tok_buf = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    state = torch.tensor([0, -1], dtype=torch.int32, device="cuda")
    rng = torch.tensor([4242, 17], dtype=torch.int32, device="cuda")
    ws = ops.sampling_ws(V, "cuda")
    for _ in range(N):
        ops.penalty_sample(d_logits, None, 1.0, None, T, top_k, 1.0, rng, tok_buf, state, 0, ws)
    torch.cuda.synchronize()
    counts = np.bincount(tok_buf[:N].cpu().numpy(), minlength=V).astype(np.float64)
    assert counts[probs == 0].sum() == 0, "a draw fell outside the top-k set"
    assert int((counts > 0).sum()) == top_k, "some of the k survivors were never drawn: truncated candidate list"
    p, cells = _chi2_p(counts, probs, N)
    print(f"[sample multi-level] {cells} cells, chi-square p = {p:.3g}")
    assert p > 1e-4, p


def test_sampling_degenerate_cases_are_the_argmax(ops):
    """top_k = 1 and T -> 0 must reproduce the greedy token every time (streaming_generate_qwen.py:99)."""
    V = 3000
    g = torch.Generator().manual_seed(3)
    logits = torch.randn(V, generator=g) * 3.0
    want = int(torch.argmax(logits))
    d_logits = logits.cuda()
    tok_buf = torch.zeros(257, dtype=torch.int32, device="cuda")
    rng = torch.tensor([1, 2], dtype=torch.int32, device="cuda")
    ws = ops.sampling_ws(V, "cuda")
    for temperature, top_k, top_p in ((0.9, 1, 1.0), (1e-3, 0, 1.0), (1e-3, 20, 0.9), (1.0, 0, 1e-6)):
        state = torch.tensor([0, -1], dtype=torch.int32, device="cuda")
        for _ in range(256):
            ops.penalty_sample(d_logits, None, 1.0, None, temperature, top_k, top_p, rng, tok_buf, state, 0, ws)
        assert (tok_buf[:256].cpu() == want).all(), (temperature, top_k, top_p)


def test_dec_lm_head_sample_distribution(ops, ref):
    """The fused decode-step form: final norm -> lm_head -> Gumbel-max candidates -> svlm_argmax_finish, 3e4 draws against
    softmax(penalised logits / T) of the kernel's own logits row."""
    from oracle import generate as og
    H, V, N, T = 256, 4096, 30_000, 0.9
    x, lnw, W = rnd((H,), 1, 1.0), rnd((H,), 2, 0.1) + 1.0, rnd((V, H), 3, 0.08)
    dx, dl, dW = x.cuda(), lnw.to(BF16).cuda(), W.cuda()
    logits = torch.zeros(V, dtype=torch.float32, device="cuda")
    ws = ops.sampling_ws(V, "cuda")
    tok_buf = torch.zeros(N + 1, dtype=torch.int32, device="cuda")
    state = torch.tensor([0, -1], dtype=torch.int32, device="cuda")
    rng = torch.tensor([99, 7], dtype=torch.int32, device="cuda")
    for _ in range(N):
        ops.dec_lm_head(dx, dl, 1e-6, dW, logits, None, 1.0, None, ws, temperature=T, rng=rng, state=state)
        ops.argmax_finish(ws, V, None, tok_buf, state, 0)
    torch.cuda.synchronize()
    probs = torch.softmax(logits.cpu() / T, dim=-1).double().numpy()
    counts = np.bincount(tok_buf[:N].cpu().numpy(), minlength=V).astype(np.float64)
    p, cells = _chi2_p(counts, probs, N)
    print(f"[dec_lm_head_sample] {cells} cells, chi-square p = {p:.3g}")
    assert p > 1e-4, p


# ----------------------------------------------------------------------------- fp8 ViT path (BASELINE configs[4])
@pytest.mark.parametrize("rows,cols", [(1024, 1280), (256, 5120), (37, 128), (3, 1024)])
def test_quant_rows_fp8_bit_exact(ops, rows, cols):
    """svlm_quant_rows_fp8 vs the oracle recipe (oracle/model.py:quant_rows_fp8): scales and e4m3 codes must be IDENTICAL."""
    from oracle import model as om
    x = rnd((rows, cols), rows + cols, 3.0)
    x[0] = 0                                       # an all-zero row keeps scale 1
    q, s = ops.quant_rows_fp8(x.cuda())
    qr, sr = om.quant_rows_fp8(x)
    assert torch.equal(s.cpu(), sr.reshape(-1))
    assert torch.equal(q.cpu().view(torch.uint8), qr.to(torch.float8_e4m3fn).view(torch.uint8))


@pytest.mark.parametrize("M,N,K,bias,res,act", [
    (1024, 3840, 1280, True, False, 0),     # ViT qkv
    (1024, 1280, 1280, True, True, 0),      # proj + residual (split-K)
    (1024, 5120, 1280, True, False, 1),     # fc1 + quick_gelu
    (1024, 1280, 5120, True, True, 0),      # fc2 + residual (split-K)
    (256, 5120, 5120, True, False, 2),      # merger + gelu
    (256, 3584, 5120, True, False, 0),      # merger -> 7B hidden
    (8192, 3840, 1280, True, False, 0),     # 8 frames per pass (dense prefill)
    (70, 256, 128, True, True, 3),          # ragged
])
def test_gemm_fp8(ops, ref, M, N, K, bias, res, act):
    """svlm_gemm_fp8 against the oracle's linear_fp8 on the same quantised operands: fp8 x fp8 products are exact in fp32, so
    only the fp32 summation order differs -- the bf16 outputs must agree to the usual one-flip bar."""
    from oracle import model as om
    A, W = rnd((M, K), 1, 1.0), rnd((N, K), 2, 0.05)
    b = rnd((N,), 3, 0.1) if bias else None
    R = rnd((M, N), 4, 1.0) if res else None
    a8, sa = ops.quant_rows_fp8(A.cuda())
    w8, sw = ops.quant_rows_fp8(W.cuda())
    got = ops.gemm_fp8(a8, sa, w8, sw, bias=None if b is None else b.cuda(), residual=None if R is None else R.cuda(), act=act)
    want = ref.gemm_fp8(a8.cpu(), sa.cpu(), w8.cpu(), sw.cpu(), bias=b, residual=R, act=act)
    close(f"gemm_fp8 {M}x{N}x{K}", got, want)
    # and what the recipe costs against the bf16 Linear it stands in for
    full = ref.gemm(A, W, bias=b, residual=R, act=act)
    err = float((want.float() - full.float()).abs().mean() / full.float().abs().mean())
    print(f"[fp8 vs bf16 linear {M}x{N}x{K}] mean relative deviation {err:.3e}")
    assert err < 0.06


def test_gemm_fp8_fused_norm(ops, ref):
    M, N, K = 1024, 1280, 1280
    A, W, b, R = rnd((M, K), 1), rnd((N, K), 2, 0.05), rnd((N,), 3, 0.1), rnd((M, N), 4)
    nw, nb = rnd((N,), 5, 0.1) + 1.0, rnd((N,), 6, 0.1)
    a8, sa = ops.quant_rows_fp8(A.cuda())
    w8, sw = ops.quant_rows_fp8(W.cuda())
    out, outn = torch.empty((M, N), dtype=BF16, device="cuda"), torch.empty((M, N), dtype=BF16, device="cuda")
    ops.gemm_fp8(a8, sa, w8, sw, bias=b.cuda(), residual=R.cuda(), out=out, norm_w=nw.to(BF16).cuda(), norm_b=nb.to(BF16).cuda(), out_norm=outn)
    o2, n2 = torch.empty((M, N), dtype=BF16), torch.empty((M, N), dtype=BF16)
    ref.gemm_fp8(a8.cpu(), sa.cpu(), w8.cpu(), sw.cpu(), bias=b, residual=R, out=o2, norm_w=nw.to(BF16), norm_b=nb.to(BF16), out_norm=n2)
    close("gemm_fp8+LN out", out, o2)
    close("gemm_fp8+LN norm", outn, n2, max_tol=2 ** -6)
    # the same call with the normalised rows leaving as the next GEMM's fp8 operand: IDENTICAL bf16 outputs, and codes + scales equal to
    # what the stand-alone quantiser makes of the kernel's own normalised rows (LayerNorm rows inside the reduce; RMSNorm rows behind it)
    for nbias in (nb.to(BF16).cuda(), None):
        out3, outn3 = torch.empty_like(out), torch.empty_like(outn)
        q8 = torch.empty((M, N), dtype=torch.float8_e4m3fn, device="cuda")
        qs = torch.empty((M,), dtype=torch.float32, device="cuda")
        ops.gemm_fp8(a8, sa, w8, sw, bias=b.cuda(), residual=R.cuda(), out=out3, norm_w=nw.to(BF16).cuda(), norm_b=nbias, out_norm=outn3,
                     out_norm_q=(q8, qs))
        if nbias is not None:
            assert torch.equal(out3, out) and torch.equal(outn3, outn)
        wq, ws_ = ops.quant_rows_fp8(outn3)
        assert torch.equal(qs, ws_) and torch.equal(q8.view(torch.uint8), wq.view(torch.uint8)), "fused quantisation differs from svlm_quant_rows_fp8"


@pytest.mark.parametrize("depth", [1, 4])
def test_vit_tower_fp8_vs_oracle_fp8_and_bf16(depth):
    """The Qwen2-VL vision tower at its REAL widths (1280 / 16 heads of 80 / 5120, merger 5120 -> 1536; 4 blocks keep the CPU oracle
    short) on the fp8 path: HIP vs the oracle with the same fp8 recipe (tight), and the recipe vs the bf16 tower (the price of fp8,
    reported; the reference has no fp8 path, so against the reference this configuration is parity-unpinned).  depth = 1 is the
    PER-BLOCK bar: one block (four fp8 Linears, two of them quantised inside the split-K reduce) + the merger."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    from oracle import model as om
    import helpers as H
    cfg = C.qwen2_vl_2b()
    cfg.vision.depth, cfg.text.num_layers = depth, 1
    sd = random_state_dict(cfg, 0, "cpu")
    eng = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=512, max_new_tokens=4, vit_fp8=True)._svlm_engine
    pix, grid = S.patchify(torch.stack([S.synthetic_frame(0, t, 448) for t in range(2)]))
    got = eng.vision_forward(pix, grid).float().cpu()
    ocfg = H.oracle_cfg(cfg)
    om.VIT_FP8 = True
    try:
        want8 = om.vit_forward(sd, ocfg, pix, grid).float()
    finally:
        om.VIT_FP8 = False
    want16 = om.vit_forward(sd, ocfg, pix, grid).float()
    sc = float(want16.abs().max())
    e_hip = float((got - want8).abs().mean()) / sc
    e_fmt = float((want8 - want16).abs().mean()) / sc
    e_hip16 = float((got - want16).abs().mean()) / sc
    print(f"[vit fp8 depth {depth}] HIP vs fp8 oracle: mean|d|/max = {e_hip:.3e}; fp8 oracle vs bf16 tower: {e_fmt:.3e}; HIP vs bf16 tower: {e_hip16:.3e}")
    # Per GEMM the two agree to bf16 flips (test_gemm_fp8).  Through a tower they cannot stay that close: a one-ulp bf16 flip in a
    # GEMM input that sits on an e4m3 rounding boundary moves that element by a whole fp8 step (6 %), so any two valid orderings
    # of the fp32 sums drift apart by a share of the quantisation noise itself.  The bars: the HIP tower is no further from the
    # fp8 oracle than the fp8 recipe is from the bf16 tower, and no further from the bf16 tower than the fp8 oracle is (+25 %).
    assert e_hip <= e_fmt + 1e-3
    assert e_hip16 <= 1.25 * e_fmt + 1e-3
    assert e_fmt <= 5e-2


# ----------------------------------------------------------------------------- device-side position bookkeeping
def test_rope_index_on_device_matches_reference_vectors(ops, golden_dir):
    """svlm_rope_index against the vectors minted from the REFERENCE's own get_rope_index (tests/golden/ref_rope_index.json, incl. a
    448x448 chunk), against the oracle on long multi-span sequences, and in its Qwen2.5 float form against the oracle's restatement
    of qwen2_5/pos_emb.py -- exact in every case (fp32 operation order included)."""
    import json, os
    from oracle import rope_index as R
    with open(os.path.join(golden_dir, "ref_rope_index.json")) as f:
        data = json.load(f)
    cases = [(name, e["ids"], e["grid"], np.asarray(e["pos"])) for name, e in data.items()]
    # a long stream: 40 chunks of (text, 256-token span), and a many-frame span (t = 5) with ragged h / w
    VS, VP, VE = 151652, 151656, 151653
    ids, grids = [1, 2, 3], []
    for c in range(40):
        ids += [10 + c, 11, VS] + [VP] * 256 + [VE, 12, 13, 14]
        grids.append([1, 32, 32])
    cases.append(("long_40", ids, grids, R.get_rope_index(ids, grids)))
    ids2 = [5, VS] + [VP] * (5 * 4 * 3) + [VE, 6, 7, VS] + [VP] * 6 + [VE]
    g2 = [[5, 8, 6], [1, 4, 6]]
    cases.append(("t5_ragged", ids2, g2, R.get_rope_index(ids2, g2)))
    cases.append(("text_only", [1, 2, 3, 4, 5], [], R.get_rope_index([1, 2, 3, 4, 5], [])))
    for name, ids, grid, want in cases:
        L, n_extra = len(ids), 7
        d_ids = torch.tensor(ids, dtype=torch.int32, device="cuda")
        d_g = torch.tensor(grid if grid else [[0, 0, 0]], dtype=torch.int32, device="cuda").reshape(-1, 3)
        ws = ops.rope_index_ws(L, len(grid), "cuda")
        pos = torch.full((3, L + n_extra + 5), -7, dtype=torch.int32, device="cuda")
        ops.rope_index(d_ids, L, d_g, len(grid), 2, VP, VS, pos, ws, n_extra=n_extra)
        got = pos.cpu().numpy()
        assert int(ws[0]) == 0, name
        assert np.array_equal(got[:, :L], want), name
        nxt = int(want.max()) + 1 if L else 0
        assert np.array_equal(got[:, L:L + n_extra], np.tile(nxt + np.arange(n_extra), (3, 1))), name       # the tokens to come
        assert (got[:, L + n_extra:] == -7).all(), name
        # float form (Qwen2.5): second_per_grid_t 0.5 and 1.0, tokens_per_second 2
        for spg in (0.5, 1.0, 0.4):
            wf = R.get_rope_index_2_5(ids, grid, 2, VP, VS, spg, 2.0)
            posf = torch.zeros((3, L + n_extra), dtype=torch.float32, device="cuda")
            ops.rope_index(d_ids, L, d_g, len(grid), 2, VP, VS, posf, ws, n_extra=n_extra, second_per_grid_t=spg, tokens_per_second=2.0)
            gf = posf.cpu().numpy()
            assert np.array_equal(gf[:, :L], wf), (name, spg)
    # the reference's failure cases surface as a status word
    bad = torch.tensor([VS, VP, VP], dtype=torch.int32, device="cuda")
    ws = ops.rope_index_ws(3, 1, "cuda")
    pos = torch.zeros((3, 8), dtype=torch.int32, device="cuda")
    ops.rope_index(bad, 3, torch.tensor([[1, 4, 4]], dtype=torch.int32, device="cuda"), 1, 2, VP, VS, pos, ws)
    assert int(ws[0]) == 4                                    # truncated vision span
    ops.rope_index(bad, 3, torch.tensor([[1, 4, 4]], dtype=torch.int32, device="cuda"), 0, 2, VP, VS, pos, ws)
    assert int(ws[0]) == 2                                    # a span without a grid row
