"""Opt-in fp8 language-model weights on the MI355X (csrc/decode_fp8.hip, SvlmEngine(llm_fp8=True)).

An llm_fp8 engine built from weights W is the bf16 model whose LLM matrices are W' = dequant(quant(W)) (power-of-two row scales,
weights.py:quantize_rows_fp8_pow2): the fp8 GEMVs compute the bf16 GEMVs on W' up to the fp32 summation order and the prefill runs
the bf16 GEMMs on W' itself.  So every kernel is held to the bars of its bf16 twin against the reference on W', and every stream to
the bars of every bf16 stream (tests/test_engine_gpu.py:_compare) against the oracle run on fp8_reference_state_dict(W)."""
import copy

import pytest
import torch

import helpers as H
from ref_ops import RefOps
from test_engine_gpu import _compare, _rel
from test_kernels_gpu import close

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16

# (H, I, Hq, Hkv): tiny, Qwen2-VL-2B, Qwen2-VL-7B, Qwen2.5-VL-3B
SHAPES = [(256, 512, 4, 2), (1536, 8960, 12, 2), (3584, 18944, 28, 4), (2048, 11008, 16, 2)]


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def q8(shape, seed, scale=0.03):
    """Random rows over four decades of magnitude (distinct scales), quantised: (q, s) on the GPU and W' on the host."""
    from streaming_vlm_amd.weights import dequantize_rows_fp8, quantize_rows_fp8_pow2
    g = torch.Generator().manual_seed(seed + 1000)
    mag = 10.0 ** (torch.rand((shape[0], 1), generator=g) * 2 - 1)
    q, s = quantize_rows_fp8_pow2((rnd(shape, seed, scale).float() * mag).to(BF16))
    return q.cuda(), s.cuda(), dequantize_rows_fp8(q, s)


def untied(cfg):
    """Config of the bf16 model fp8_reference_state_dict describes: its lm_head.weight is a matrix of its own."""
    cfg = copy.deepcopy(cfg)
    cfg.text.tie_word_embeddings = False
    return cfg


@pytest.mark.parametrize("H,I,Hq,Hkv", SHAPES)
def test_fp8_decode_kernels_vs_reference_on_dequantised_weights(ops, H, I, Hq, Hkv):
    ref = RefOps()
    D = 128
    qd, kd = Hq * D, Hkv * D
    x, lnw = rnd((H,), 1, 2.0), rnd((H,), 2, 0.1) + 1
    # --- norm + qkv + append (device-side length)
    W8, s8, Wp = q8((qd + 2 * kd, H), 3)
    b = rnd((qd + 2 * kd,), 4, 0.1)
    pool_c = rnd((2, 2, Hkv, 48, D), 5)
    pool_g = pool_c.clone().cuda()
    slot_of = torch.randperm(48, generator=torch.Generator().manual_seed(6)).to(torch.int32)
    q_c, q_g = torch.zeros(qd + 2 * kd, dtype=BF16), torch.zeros(qd + 2 * kd, dtype=BF16, device="cuda")
    ref.dec_qkv(x, lnw, 1e-6, Wp, b, q_c, pool_c, 1, slot_of, qd, kd, length=17)
    len_dev = torch.tensor([17], dtype=torch.int32, device="cuda")
    ops.dec_qkv_fp8(x.cuda(), lnw.cuda(), 1e-6, W8, s8, b.cuda(), q_g, pool_g, 1, slot_of.cuda(), qd, kd, len_dev=len_dev)
    close("dec_qkv_fp8 q", q_g[:qd], q_c[:qd])
    close("dec_qkv_fp8 pool", pool_g, pool_c)
    assert torch.equal(pool_g.cpu()[0], pool_c[0]), "other layers untouched"
    # the same launch with a host-side length writes the same row
    pool_h = rnd((2, 2, Hkv, 48, D), 5).cuda()
    ops.dec_qkv_fp8(x.cuda(), lnw.cuda(), 1e-6, W8, s8, b.cuda(), q_g, pool_h, 1, slot_of.cuda(), qd, kd, length=17)
    assert torch.equal(pool_h, pool_g)
    # --- norm + gate/up + SwiGLU
    Wgu8, sgu, Wgup = q8((2 * I, H), 7)
    h_c, h_g = torch.zeros(I, dtype=BF16), torch.zeros(I, dtype=BF16, device="cuda")
    ref.dec_gate_up(x, lnw, 1e-6, Wgup, h_c)
    ops.dec_gate_up_fp8(x.cuda(), lnw.cuda(), 1e-6, Wgu8, sgu, h_g)
    close("dec_gate_up_fp8", h_g, h_c)
    # --- o_proj and down_proj + residual (short and long reductions: both K-split forms)
    for name, N, K, seed in (("o_proj", H, qd, 10), ("down_proj", H, I, 11)):
        Wo8, so, Wop = q8((N, K), seed)
        a, res = rnd((K,), seed + 1, 1.0), rnd((N,), seed + 2, 1.0)
        y_c = ref.gemv(a, Wop, residual=res, out=torch.empty(N, dtype=BF16))
        y_g = ops.gemv_fp8(a.cuda(), Wo8, so, residual=res.cuda(), out=torch.empty(N, dtype=BF16, device="cuda"))
        close(f"gemv_fp8 {name} {N}x{K}", y_g, y_c)
    # --- final norm + lm_head + penalty + argmax candidates + feedback; prefill's fp32 last-row logits
    V = 151936 if H == 1536 else 20011
    Wl8, sl8, Wlp = q8((V, H), 8)
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
    ref.dec_lm_head(x, lnw, 1e-6, Wlp, lg_c, seen_c, 1.05, sup, None)
    ref.argmax_finish(None, V, seen_c, tb_c, st_c, 1)
    ops.dec_lm_head_fp8(x.cuda(), lnw.cuda(), 1e-6, Wl8, sl8, lg_g, seen_g, 1.05, sup.cuda(), sws)
    ops.argmax_finish(sws, V, seen_g, tb_g, st_g, 1)
    close("dec_lm_head_fp8 logits", lg_g, lg_c)
    sc = lg_g.cpu().clone()
    m = torch.zeros(V, dtype=torch.uint8)
    ref.mark_seen(ids, 300, m)
    mm = m.bool()
    sc[mm] = torch.where(sc[mm] < 0, sc[mm] * 1.05, sc[mm] / 1.05)
    sc[sup.long()] = float("-inf")
    assert int(tb_g[1]) == int(torch.argmax(sc)), "fused argmax != argmax of its own logits"
    assert torch.equal(st_g.cpu(), st_c)
    xn = rnd((H,), 12, 1.0)
    f_c = ref.gemv(xn, Wlp, out_f32=torch.zeros(V))
    f_g = ops.gemv_fp8(xn.cuda(), Wl8, sl8, out_f32=torch.zeros(V, device="cuda"))
    close("gemv_fp8 lm_head fp32", f_g, f_c)
    # --- temperature sampling form: same logits, a token drawn among them
    lg2 = torch.zeros(V, device="cuda")
    rng = torch.tensor([123, 456], dtype=torch.int32, device="cuda")
    st2 = torch.tensor([50, 0], dtype=torch.int32, device="cuda")
    ops.dec_lm_head_fp8(x.cuda(), lnw.cuda(), 1e-6, Wl8, sl8, lg2, None, 1.0, None, sws, temperature=0.7, rng=rng, state=st2)
    ops.argmax_finish(sws, V, None, tb_g, st2, 1)
    assert torch.equal(lg2, lg_g) and 0 <= int(tb_g[1]) < V
    # --- dequantisation: W' bit for bit
    out = torch.empty((2 * I, H), dtype=BF16, device="cuda")
    assert torch.equal(ops.dequant_fp8(Wgu8, sgu, out).cpu(), Wgup)


def test_fp8_gemv_over_every_e4m3_code_is_exact(ops):
    """All 254 finite OCP e4m3 codes (subnormals and +-0 included; 0x7F / 0xFF are NaN): row r holds code (j + r) mod 256 at column j
    (NaN codes zeroed), x is one-hot, so every output is ONE product q * x * s -- exact in fp32 and in bf16.  Several columns (every
    byte position of a 16-B load, two lanes) and several scales.  A conversion that flushes subnormals or reads the FNUZ encoding
    (bias 8, no negative zero) fails here."""
    K = N = 256
    r = torch.arange(N).view(N, 1)
    codes = ((torch.arange(K).view(1, K) + r) % 256).to(torch.uint8)
    codes[(codes == 0x7F) | (codes == 0xFF)] = 0
    q = codes.view(torch.float8_e4m3fn)
    vals = q.float()
    assert int(torch.isfinite(vals).sum()) == N * K and len(set(vals.flatten().tolist())) == 253    # 254 codes, +0 == -0
    for s_exp in (0, -10, 4, -20):
        s = torch.full((N,), 2.0 ** s_exp)
        for j in (0, 1, 2, 3, 5, 14, 15, 16, 200, 255):
            xv = 2.0 ** (j % 5 - 2)
            x = torch.zeros(K, dtype=BF16)
            x[j] = xv
            want = vals[:, j] * xv * s
            got = ops.gemv_fp8(x.cuda(), q.cuda(), s.cuda(), out_f32=torch.zeros(N, device="cuda")).cpu()
            assert torch.equal(got, want), (s_exp, j, (got - want).abs().max())
            gotb = ops.gemv_fp8(x.cuda(), q.cuda(), s.cuda()).cpu()
            assert torch.equal(gotb.float(), want), (s_exp, j)
        w = ops.dequant_fp8(q.cuda(), s.cuda(), torch.empty((N, K), dtype=BF16, device="cuda")).cpu()
        assert torch.equal(w.float(), vals * s.view(N, 1)), s_exp


def _fp8_model(family="qwen2", stream=None, use_graph=True, **kw):
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import fp8_reference_state_dict
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg, **(stream or {}))
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8, use_graph=use_graph,
                               llm_fp8=True, **kw)
    assert model._svlm_engine.llm_fp8
    return cfg, sd, fp8_reference_state_dict(sd, cfg), model


def test_fp8_stream_sink_window_and_the_price_of_fp8():
    """The bars of every bf16 stream against the oracle on W'; then the distance of the fp8 model from the bf16 model on W (reported)."""
    import streaming_vlm_amd as S
    cfg, sd, sdp, model = _fp8_model()
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
    print(f"[price of fp8] tiny decisive stream, fp8 vs bf16 model on W: logits max rel {worst_max:.3e} mean rel {worst_mean:.3e}, "
          f"greedy tokens {same}/{sum(len(x['own']) for x in a)} equal; vs the oracle on W' (the model it is): mean rel {out['worst_mean']:.3e}")


def test_fp8_streams_qwen2_5_structural_and_all_text():
    cfg, sd, sdp, model = _fp8_model(family="qwen2_5")
    _compare(untied(cfg), sdp, 7, model, policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8,
             previous_text="a b c d e f g h i j k l m n o p")
    cfg, sd, sdp, model = _fp8_model(family="qwen2_5", stream=dict(all_text=True))
    _compare(untied(cfg), sdp, 4, model, all_text=True)


def test_fp8_graph_replay_equals_eager_launches():
    logs = []
    for g in (True, False):
        cfg, sd, sdp, model = _fp8_model(use_graph=g)
        logs.append(H.run_engine_stream(model, 4, keep_logits=True)[3])
    for a, b in zip(*logs):
        assert a["ids"] == b["ids"]
        for x, y in zip(a["logits"], b["logits"]):
            assert torch.equal(x, y)


def test_fp8_llm_with_the_fp8_vision_tower():
    """vit_fp8 and llm_fp8 together (a Qwen2 tower of widths that are multiples of 128: 8 heads of 80).  Against the vit_fp8 engine
    with the bf16 LLM on W' (same tower, same bits; the LLM differs by summation order only): exact greedy tokens, logits within the
    bf16 noise of a stream."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import fp8_reference_state_dict
    cfg = C.tiny()
    cfg.vision.embed_dim, cfg.vision.num_heads, cfg.vision.mlp_hidden = 640, 8, 1280
    sd = H.decisive_weights(cfg)
    sdp = fp8_reference_state_dict(sd, cfg)
    both = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8, vit_fp8=True, llm_fp8=True)
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
    print(f"[vit_fp8 + llm_fp8] vs vit_fp8 with the bf16 LLM on W': logits max rel {worst_max:.3e} mean rel {worst_mean:.3e}")
    assert worst_mean <= 5e-3 and worst_max <= 5e-2


def test_fp8_engine_memory_at_7b_widths():
    """Two layers at the Qwen2-VL-7B widths (untied lm_head): the fp8 build holds its layer matrices and lm_head in <= 0.55x the bytes the
    bf16 build's take (codes + row scales; the prefill's bf16 scratch layer is allocated by the first prefill, not at build)."""
    import gc
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    cfg = C.qwen2_vl_7b()
    cfg.text.num_layers, cfg.vision.depth = 2, 1
    sd = {k: v.cuda() for k, v in random_state_dict(cfg, 0, "cpu").items()}
    torch.cuda.synchronize()
    delta = {}
    for fp8 in (False, True):
        gc.collect()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        m = S.StreamingQwen2VL(cfg, sd, "cuda", max_len=512, max_new_tokens=4, llm_fp8=fp8)
        torch.cuda.synchronize()
        delta[fp8] = torch.cuda.memory_allocated() - base
        if not fp8:
            w = m._svlm_engine.w
            flat16 = sum(l["flat"].numel() * 2 for l in w.layers)
            big = flat16 + w.lm_head.numel() * 2
            # (the bf16 build takes a device tensor of the right dtype over without a copy: then its lm_head costs it nothing new)
            new16 = flat16 + (0 if w.lm_head.data_ptr() == sd["lm_head.weight"].data_ptr() else w.lm_head.numel() * 2)
        del m
    fp8_big = delta[True] - (delta[False] - new16)      # what the fp8 build allocates beyond what both builds share
    print(f"[fp8 memory] 2 layers at 7B widths + lm_head: bf16 {big / 2**20:.0f} MiB, fp8 {fp8_big / 2**20:.0f} MiB ({fp8_big / big:.3f}x)")
    assert fp8_big <= 0.55 * big
