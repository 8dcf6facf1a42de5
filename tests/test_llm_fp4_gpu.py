"""Opt-in MXFP4 language-model weights on the MI355X (csrc/decode_fp4.hip, SvlmEngine(llm_fp4=True)).

An llm_fp4 engine built from weights W is the bf16 model whose LLM layer matrices are W' = dequant(quant(W)) (OCP e2m1 codes with one
power-of-two scale per block of 32, weights.py:quantize_blocks_mxfp4) and whose lm_head is the e4m3 W' of the fp8 engine: the fp4 GEMVs
compute the bf16 GEMVs on W' up to the fp32 summation order and the prefill runs the bf16 GEMMs on W' itself.  So every kernel is held
to the bars of its bf16 twin against the reference on W', and every stream to the bars of every bf16 stream
(tests/test_engine_gpu.py:_compare) against the oracle run on fp4_reference_state_dict(W)."""
import copy

import pytest
import torch

import helpers as H
from ref_ops import RefOps
from test_engine_gpu import _compare, _rel
from test_kernels_gpu import close
from test_llm_fp8_gpu import SHAPES

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def q4(shape, seed, scale=0.03):
    """Random rows AND blocks over four decades of magnitude (neighbouring blocks carry different scales), quantised on the GPU:
    (codes, scales) there and W' on the host."""
    from streaming_vlm_amd.weights import dequantize_blocks_mxfp4, quantize_blocks_mxfp4
    N, K = shape
    g = torch.Generator(device="cuda").manual_seed(seed + 2000)
    w = torch.randn(shape, generator=g, device="cuda") * scale
    mag = 10.0 ** (torch.rand((N, 1, 1), generator=g, device="cuda") * 2 - 1 + torch.rand((N, K // 32, 1), generator=g, device="cuda") * 2 - 1)
    codes, scales = quantize_blocks_mxfp4((w.view(N, K // 32, 32) * mag).view(N, K).to(BF16))
    assert int(scales.max()) - int(scales.min()) >= 10
    return codes, scales, dequantize_blocks_mxfp4(codes, scales).cpu()


def untied(cfg):
    """Config of the bf16 model fp4_reference_state_dict describes: its lm_head.weight is a matrix of its own."""
    cfg = copy.deepcopy(cfg)
    cfg.text.tie_word_embeddings = False
    return cfg


@pytest.mark.parametrize("H,I,Hq,Hkv", SHAPES)
def test_fp4_decode_kernels_vs_reference_on_dequantised_weights(ops, H, I, Hq, Hkv):
    """K below one K-step of 2048 (256, 512, 1536), a whole one (2048), ragged last K-steps (3584, 8960, 11008, 18944); both K-split
    forms of the residual GEMV; both length forms of dec_qkv_fp4."""
    ref = RefOps()
    D = 128
    qd, kd = Hq * D, Hkv * D
    x, lnw = rnd((H,), 1, 2.0), rnd((H,), 2, 0.1) + 1
    # --- norm + qkv + append (device-side length)
    W4, s4, Wp = q4((qd + 2 * kd, H), 3)
    b = rnd((qd + 2 * kd,), 4, 0.1)
    pool_c = rnd((2, 2, Hkv, 48, D), 5)
    pool_g = pool_c.clone().cuda()
    slot_of = torch.randperm(48, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    q_c, q_g = torch.zeros(qd + 2 * kd, dtype=BF16), torch.zeros(qd + 2 * kd, dtype=BF16, device="cuda")
    ref.dec_qkv(x, lnw, 1e-6, Wp, b, q_c, pool_c, 1, slot_of, qd, kd, length=17)
    len_dev = torch.tensor([17], dtype=torch.int32, device="cuda")
    ops.dec_qkv_fp4(x.cuda(), lnw.cuda(), 1e-6, W4, s4, b.cuda(), q_g, pool_g, 1, slot_of.cuda(), qd, kd, len_dev=len_dev)
    close("dec_qkv_fp4 q", q_g[:qd], q_c[:qd])
    close("dec_qkv_fp4 pool", pool_g, pool_c)
    assert torch.equal(pool_g.cpu()[0], pool_c[0]), "other layers untouched"
    # the same launch with a host-side length writes the same row
    pool_h = rnd((2, 2, Hkv, 48, D), 5).cuda()
    ops.dec_qkv_fp4(x.cuda(), lnw.cuda(), 1e-6, W4, s4, b.cuda(), q_g, pool_h, 1, slot_of.cuda(), qd, kd, length=17)
    assert torch.equal(pool_h, pool_g)
    # --- norm + gate/up + SwiGLU
    Wgu4, sgu, Wgup = q4((2 * I, H), 7)
    h_c, h_g = torch.zeros(I, dtype=BF16), torch.zeros(I, dtype=BF16, device="cuda")
    ref.dec_gate_up(x, lnw, 1e-6, Wgup, h_c)
    ops.dec_gate_up_fp4(x.cuda(), lnw.cuda(), 1e-6, Wgu4, sgu, h_g)
    close("dec_gate_up_fp4", h_g, h_c)
    # --- o_proj and down_proj + residual (short and long reductions: both K-split forms)
    for name, N, K, seed in (("o_proj", H, qd, 10), ("down_proj", H, I, 11)):
        Wo4, so, Wop = q4((N, K), seed)
        a, res = rnd((K,), seed + 1, 1.0), rnd((N,), seed + 2, 1.0)
        y_c = ref.gemv(a, Wop, residual=res, out=torch.empty(N, dtype=BF16))
        y_g = ops.gemv_fp4(a.cuda(), Wo4, so, residual=res.cuda(), out=torch.empty(N, dtype=BF16, device="cuda"))
        close(f"gemv_fp4 {name} {N}x{K}", y_g, y_c)
    # --- dequantisation: W' bit for bit
    out = torch.empty((2 * I, H), dtype=BF16, device="cuda")
    assert torch.equal(ops.dequant_fp4(Wgu4, sgu, out).cpu(), Wgup)


@pytest.mark.parametrize("N,K", [(37, 2112), (4099, 2112), (1541, 4160), (13, 96)])
def test_fp4_kernels_at_row_counts_that_are_no_multiple_of_a_workgroup(ops, N, K):
    """N not a multiple of a workgroup's rows in each form of svlm_gemv_fp4 (1 row per wave, 2 rows per wave, 2 rows with K split over
    4 waves -- there also K / 32 not a multiple of 4) and in svlm_dec_gate_up_fp4, with bias and the fp32 output; the rows past N are
    never written."""
    ref = RefOps()
    W4, s4, Wp = q4((N, K), 20 + N)
    a, res, bias = rnd((K,), 21, 1.0), rnd((N,), 22, 1.0), rnd((N,), 23, 0.5)
    y_c = ref.gemv(a, Wp, bias=bias, residual=res, out=torch.empty(N, dtype=BF16))
    guard = torch.full((N + 8,), 7.0, dtype=BF16, device="cuda")
    ops.gemv_fp4(a.cuda(), W4, s4, bias=bias.cuda(), residual=res.cuda(), out=guard[:N])
    close(f"gemv_fp4 {N}x{K}", guard[:N], y_c)
    assert bool((guard[N:] == 7.0).all())
    f_c = ref.gemv(a, Wp, out_f32=torch.zeros(N))
    f_g = ops.gemv_fp4(a.cuda(), W4, s4, out_f32=torch.zeros(N, device="cuda"))
    close(f"gemv_fp4 fp32 {N}x{K}", f_g, f_c)
    # the fused gate/up kernel at I = N gate rows; K = 4160 takes its form for rows above 4096 (a second batch of K-steps)
    Wgu4, sgu, Wgup = q4((2 * N, K), 30 + N)
    x, lnw = rnd((K,), 1, 2.0), rnd((K,), 2, 0.1) + 1
    h_c = torch.zeros(N, dtype=BF16)
    h_g = torch.full((N + 8,), 7.0, dtype=BF16, device="cuda")
    ref.dec_gate_up(x, lnw, 1e-6, Wgup, h_c)
    ops.dec_gate_up_fp4(x.cuda(), lnw.cuda(), 1e-6, Wgu4, sgu, h_g[:N])
    close(f"dec_gate_up_fp4 I={N}", h_g[:N], h_c)
    assert bool((h_g[N:] == 7.0).all())


def test_fp4_gemv_over_every_e2m1_code_and_position_is_exact(ops):
    """All 16 codes at every position: row r holds nibble (j + r) mod 16 at column j, x is one-hot, so every output is ONE product
    code * x * 2^e -- exact in fp32 and in bf16.  Columns: every nibble position of one 16-B load (0..31), the first and last column of
    a block, a second lane (32..63) and later blocks; uniform scales 2^0, 2^-10, 2^4, 2^-20.  A swapped nibble order, a wrong exponent
    bias or a mis-scaled conversion fails here (-0 == +0 aside)."""
    K = N = 256
    r = torch.arange(N).view(N, 1)
    nib = ((torch.arange(K).view(1, K) + r) % 16).to(torch.uint8)
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    vals = torch.tensor(E2M1 + [-v for v in E2M1])[nib.long()]
    for s_exp in (0, -10, 4, -20):
        s = torch.full((N, K // 32), 127 + s_exp, dtype=torch.uint8)
        sf = 2.0 ** s_exp
        for j in list(range(32)) + [32, 33, 63, 64, 95, 224, 255]:
            xv = 2.0 ** (j % 5 - 2)
            x = torch.zeros(K, dtype=BF16)
            x[j] = xv
            want = vals[:, j] * xv * sf
            got = ops.gemv_fp4(x.cuda(), codes.cuda(), s.cuda(), out_f32=torch.zeros(N, device="cuda")).cpu()
            assert torch.equal(got, want), (s_exp, j, (got - want).abs().max())
            gotb = ops.gemv_fp4(x.cuda(), codes.cuda(), s.cuda()).cpu()
            assert torch.equal(gotb.float(), want), (s_exp, j)
        w = ops.dequant_fp4(codes.cuda(), s.cuda(), torch.empty((N, K), dtype=BF16, device="cuda")).cpu()
        assert torch.equal(w.float(), vals * sf), s_exp


@pytest.mark.parametrize("N,K", [(3, 2048 + 64), (3, 4096 + 64)])
def test_fp4_scale_indexing_block_by_block(ops, N, K):
    """Every block of a row carries its own exponent (pairwise distinct within the row), every code is 1.0, x is all-ones on ONE block:
    the output is exactly 32 * 2^e of that block.  K = 2048 + 64: the last K-step holds two live lanes; K = 4096 + 64: the form that
    splits K over four waves (K / 32 = 130 blocks, 33 per wave, the last wave 31)."""
    nb = K // 32
    e = (torch.arange(nb).view(1, nb) * 7 % nb + torch.arange(N).view(N, 1) * 3 - 60).to(torch.int32)        # 7 is coprime to 66 and 130
    assert all(len(set(row.tolist())) == nb for row in e)
    scales = (e + 127).to(torch.uint8).cuda()
    codes = torch.full((N, K // 2), 0x22, dtype=torch.uint8, device="cuda")
    for b in range(nb):
        x = torch.zeros(K, dtype=BF16)
        x[32 * b:32 * b + 32] = 1.0
        want = 32.0 * torch.pow(2.0, e[:, b].float())
        got = ops.gemv_fp4(x.cuda(), codes, scales, out_f32=torch.zeros(N, device="cuda")).cpu()
        assert torch.equal(got, want), (b, got, want)
    w = ops.dequant_fp4(codes, scales, torch.empty((N, K), dtype=BF16, device="cuda")).cpu().float()
    assert torch.equal(w, torch.pow(2.0, e.float()).repeat_interleave(32, dim=1))


def _fp4_model(family="qwen2", stream=None, use_graph=True, **kw):
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import fp4_reference_state_dict
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg, **(stream or {}))
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8, use_graph=use_graph,
                               llm_fp4=True, **kw)
    assert model._svlm_engine.llm_fp4
    return cfg, sd, fp4_reference_state_dict(sd, cfg), model


def test_fp4_stream_sink_window_and_the_price_of_fp4():
    """The bars of every bf16 stream against the oracle on W'; then the distance of the fp4 model from the bf16 model on W (reported)."""
    import streaming_vlm_amd as S
    cfg, sd, sdp, model = _fp4_model()
    out = _compare(untied(cfg), sdp, 6, model)
    assert out["same"] == out["steps"]
    ref = H.run_oracle_stream(cfg, sdp, 3, keep_logits=True)
    bf = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8)
    a = H.run_engine_stream(model, 3, keep_logits=True, force_tokens=ref["generated"])[3]
    b = H.run_engine_stream(bf, 3, keep_logits=True, force_tokens=ref["generated"])[3]
    worst_max = worst_mean = 0.0
    for x, y in zip(a, b):
        for u, v in zip(x["logits"], y["logits"]):
            mx, mn = _rel(u, v)
            worst_max, worst_mean = max(worst_max, mx), max(worst_mean, mn)
    same = sum(int(p == q) for x, y in zip(a, b) for p, q in zip(x["own"], y["own"]))
    print(f"[price of fp4] tiny decisive stream, fp4 vs bf16 model on W: logits max rel {worst_max:.3e} mean rel {worst_mean:.3e}, "
          f"greedy tokens {same}/{sum(len(x['own']) for x in a)} equal; vs the oracle on W' (the model it is): mean rel {out['worst_mean']:.3e}")


def test_fp4_stream_qwen2_5_structural():
    cfg, sd, sdp, model = _fp4_model(family="qwen2_5")
    _compare(untied(cfg), sdp, 7, model, policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8,
             previous_text="a b c d e f g h i j k l m n o p")


def test_fp4_stream_qwen2_5_all_text():
    cfg, sd, sdp, model = _fp4_model(family="qwen2_5", stream=dict(all_text=True))
    _compare(untied(cfg), sdp, 4, model, all_text=True)


def test_fp4_graph_replay_equals_eager_launches():
    logs = []
    for g in (True, False):
        cfg, sd, sdp, model = _fp4_model(use_graph=g)
        logs.append(H.run_engine_stream(model, 4, keep_logits=True)[3])
    for a, b in zip(*logs):
        assert a["ids"] == b["ids"]
        for x, y in zip(a["logits"], b["logits"]):
            assert torch.equal(x, y)


def test_fp4_llm_with_the_fp8_vision_tower():
    """vit_fp8 and llm_fp4 together.  Against the vit_fp8 engine with the bf16 LLM on W' (same tower, same bits; the LLM differs by
    summation order only): exact greedy tokens, logits within the bf16 noise of a stream (the bars of the fp8 test)."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import fp4_reference_state_dict
    cfg = C.tiny()
    cfg.vision.embed_dim, cfg.vision.num_heads, cfg.vision.mlp_hidden = 640, 8, 1280
    sd = H.decisive_weights(cfg)
    sdp = fp4_reference_state_dict(sd, cfg)
    both = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8, vit_fp8=True, llm_fp4=True)
    vit = S.StreamingQwen2VL(untied(cfg), {k: v.cuda() for k, v in sdp.items()}, "cuda", max_len=768, max_new_tokens=8, vit_fp8=True)
    a = H.run_engine_stream(both, 4, keep_logits=True)
    b = H.run_engine_stream(vit, 4, keep_logits=True)
    assert a[1] == b[1]
    worst_max = worst_mean = 0.0
    for x, y in zip(a[3], b[3]):
        assert x["ids"] == y["ids"] and x["kv_len"] == y["kv_len"]
        for u, v in zip(x["logits"], y["logits"]):
            mx, mn = _rel(u, v)
            worst_max, worst_mean = max(worst_max, mx), max(worst_mean, mn)
    print(f"[vit_fp8 + llm_fp4] vs vit_fp8 with the bf16 LLM on W': logits max rel {worst_max:.3e} mean rel {worst_mean:.3e}")
    assert worst_mean <= 5e-3 and worst_max <= 5e-2


def test_fp4_engine_memory_at_7b_widths():
    """Two layers at the Qwen2-VL-7B widths: the fp4 build allocates at most what the fp8 build does minus 0.4 B per layer-matrix weight
    (the format saves 1 - 0.53125 = 0.469 B per weight against e4m3; the margin leaves room for allocator rounding).  Both keep the same
    e4m3 lm_head; the prefill's bf16 scratch layer is allocated by the first prefill, not at build."""
    import gc
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    cfg = C.qwen2_vl_7b()
    cfg.text.num_layers, cfg.vision.depth = 2, 1
    sd = {k: v.cuda() for k, v in random_state_dict(cfg, 0, "cpu").items()}
    torch.cuda.synchronize()
    delta = {}
    for fmt in ("llm_fp8", "llm_fp4"):
        gc.collect()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        m = S.StreamingQwen2VL(cfg, sd, "cuda", max_len=512, max_new_tokens=4, **{fmt: True})
        torch.cuda.synchronize()
        gc.collect()
        delta[fmt] = torch.cuda.memory_allocated() - base
        if fmt == "llm_fp8":
            n_w = sum(l["flat8"].numel() for l in m._svlm_engine.w.layers)
        del m
    print(f"[fp4 memory] 2 layers at 7B widths ({n_w / 2**20:.0f} Mi weights): fp8 build {delta['llm_fp8'] / 2**20:.0f} MiB, "
          f"fp4 build {delta['llm_fp4'] / 2**20:.0f} MiB, saving {(delta['llm_fp8'] - delta['llm_fp4']) / n_w:.3f} B per weight")
    assert delta["llm_fp4"] <= delta["llm_fp8"] - 0.4 * n_w
