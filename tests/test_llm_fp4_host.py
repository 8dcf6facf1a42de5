"""Opt-in MXFP4 language-model weights, host side (no GPU): the block quantiser (OCP e2m1 codes, e8m0 scales), the bf16 reference
image W' of an fp4 model, and the engine's sequencing of the fp4 decode step and dequantising prefill on the CPU reference backend --
which must be the bf16 engine on W', bit for bit."""
import copy
from types import SimpleNamespace

import pytest
import torch

import helpers as H
from ref_ops import RefOps
from ref_ops_fp4 import RefOpsFp4
from ref_ops_fp8 import RefOpsFp8

import streaming_vlm_amd as S
from streaming_vlm_amd import config as C
from streaming_vlm_amd.engine import SvlmEngine
from streaming_vlm_amd.stream_group import StreamGroup
from streaming_vlm_amd.weights import (L_PREFIX, LLM_FP8_MATRICES, dequantize_blocks_mxfp4, dequantize_rows_fp8, fp4_reference_state_dict,
                                       quantize_blocks_mxfp4, quantize_rows_fp8_pow2, random_state_dict)

BF16 = torch.bfloat16
E2M1 = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]


def _w(shape=(64, 384), seed=0, decades=4.0):
    """Random blocks over `decades` decades of magnitude, so neighbouring blocks carry different scales."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(shape, generator=g) * 0.02
    mag = 10.0 ** (torch.rand((shape[0], shape[1] // 32, 1), generator=g) * decades - decades / 2)
    return (w.view(shape[0], -1, 32) * mag).view(shape).to(BF16)


def _unpack(codes):
    """[N, K / 2] bytes -> [N, K] nibbles in element order (element 2i = low nibble of byte i)."""
    return torch.stack([codes & 0xF, codes >> 4], dim=-1).view(codes.shape[0], -1)


def test_quantiser_scale_bytes_and_codes_never_saturate():
    w = _w()
    w[3] *= 2.0 ** 100              # loud and quiet rows: the ends of the scale range
    w[4] *= 2.0 ** -100
    codes, scales = quantize_blocks_mxfp4(w)
    assert codes.dtype == torch.uint8 and scales.dtype == torch.uint8 and codes.shape == (64, 192) and scales.shape == (64, 12)
    assert int(scales.min()) >= 2 and int(scales.max()) <= 252
    amax = w.float().view(64, 12, 32).abs().amax(2).double()
    s = torch.pow(2.0, scales.double() - 127)
    assert bool((amax <= 6 * s).all()), "no code saturates"
    unclamped = scales > 2
    assert bool((amax > 3 * s)[unclamped & (amax > 0)].all()), "the smallest such scale: half of it would saturate"
    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_blocks_mxfp4(torch.zeros(4, 48, dtype=BF16))
    loud = torch.zeros(1, 32, dtype=BF16)
    loud[0, 0] = 2.0 ** 127 * 1.75                     # > 6 * 2^125
    with pytest.raises(ValueError, match="2\\^125"):
        quantize_blocks_mxfp4(loud)
    quiet = torch.zeros(1, 32, dtype=BF16)
    quiet[0, 0], quiet[0, 1] = 2.0 ** -126, 2.0 ** -130          # below 0.5 * 2^-125 = the smallest W': e stays -125, toward zero
    c, sc = quantize_blocks_mxfp4(quiet)
    assert int(sc[0, 0]) == 2 and _unpack(c)[0, :2].tolist() == [1, 0]
    assert float(dequantize_blocks_mxfp4(c, sc)[0, 0]) == 2.0 ** -126


def test_zero_blocks_exact_amax_and_ties_to_even():
    w = torch.zeros(4, 64, dtype=BF16)
    w[1, 0] = -6 * 2.0 ** -9                            # amax exactly 6 * 2^j keeps e = j
    w[1, 32] = 6 * 2.0 ** -9 * 1.0078125                # one bf16 step above: the next scale
    w[2, :8] = torch.tensor([2.5, 5.0, 1.25, 1.75, 6.0, -0.25, 0.75, 3.5])
    w[3, :4] = torch.tensor([-2.5, -5.0, -1.25, -6.0])
    codes, scales = quantize_blocks_mxfp4(w)
    nib = _unpack(codes)
    assert scales[0].tolist() == [127, 127] and int(codes[0].max()) == 0, "all-zero blocks: e = 0, codes 0"
    assert scales[1].tolist() == [127 - 9, 127 - 8] and int(nib[1, 0]) == 0xF and int(nib[1, 32]) == 5
    wp = dequantize_blocks_mxfp4(codes, scales).float()
    assert wp[2, :8].tolist() == [2.0, 4.0, 1.0, 2.0, 6.0, 0.0, 1.0, 4.0]
    assert nib[2, :8].tolist() == [4, 6, 2, 4, 7, 0, 2, 6], "ties go to the even code; a rounded-away negative is +0"
    assert wp[3, :4].tolist() == [-2.0, -4.0, -1.0, -6.0] and nib[3, :4].tolist() == [12, 14, 10, 15]
    assert int(scales.max()) < 0xFF, "0xFF (NaN) is never produced"


def test_nibble_order_and_scale_layout_on_a_hand_written_row():
    """Element 2i is the LOW nibble of byte i; the scale byte of block b is e + 127, row-major in an array of its own."""
    row = torch.zeros(1, 64)
    row[0, :16] = torch.tensor(E2M1 + [-v for v in E2M1])        # codes 0..15 in order (-0 quantises to +0: code 0)
    row[0, 32:36] = torch.tensor([6.0, -3.0, 0.5, 1.5]) * 2.0 ** 5
    codes, scales = quantize_blocks_mxfp4(row.to(BF16))
    assert codes[0, :8].tolist() == [0x10, 0x32, 0x54, 0x76, 0x90, 0xBA, 0xDC, 0xFE]
    assert codes[0, 16:18].tolist() == [0xD7, 0x31] and scales.tolist() == [[127, 132]]
    hand_codes = torch.tensor([[0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE] + [0] * 8 + [0xD7, 0x31] + [0] * 14], dtype=torch.uint8)
    wp = dequantize_blocks_mxfp4(hand_codes, torch.tensor([[127, 132]], dtype=torch.uint8)).float()
    assert torch.equal(wp, row) and str(float(wp[0, 8])) == "-0.0"


def test_dequantised_weights_are_exact_in_bf16_and_a_fixed_point():
    """W' = code * 2^e is exact in bf16 and quantising it again gives W' again.  The codes and scales themselves come back unchanged
    except where a block's largest code is 3 (amax / 2^e in (3, 3.5] rounded down): then amax(W') = 3 * 2^e = 6 * 2^(e - 1), the
    smallest-scale rule takes e - 1 and every code of the block one binade up -- the same W' under another name."""
    for seed, decades in ((0, 4.0), (1, 0.0), (2, 8.0)):
        w = _w((128, 512), seed, decades)
        codes, scales = quantize_blocks_mxfp4(w)
        nib = _unpack(codes).view(128, 16, 32)
        wf = torch.tensor(E2M1 + [-v for v in E2M1])[nib.long()] * torch.pow(2.0, scales.float() - 127).unsqueeze(2)
        wp = dequantize_blocks_mxfp4(codes, scales)
        assert torch.equal(wp.float(), wf.view(128, 512)) and torch.equal(wp.float().to(BF16), wp)
        codes2, scales2 = quantize_blocks_mxfp4(wp)
        assert torch.equal(dequantize_blocks_mxfp4(codes2, scales2), wp)
        top = (nib & 7).amax(2)
        same_s = scales2 == scales
        same_c = (_unpack(codes2).view(128, 16, 32) == nib).all(2)
        assert bool((same_s == same_c).all()) and bool(same_s[top >= 6].all()) and bool(same_s[top == 0].all())
        assert bool((scales2[~same_s].int() == scales[~same_s].int() - 1).all()) and bool((top[~same_s] == 5).all())
        assert int(same_s.sum()) > 0.7 * same_s.numel()
        # the GEMV with the scale inside the product is the bf16 GEMV on W': same order, same bits
        x = torch.randn(512, generator=torch.Generator().manual_seed(seed)).to(BF16).float()
        assert torch.equal(wf.view(128, 512) @ x, wp.float() @ x)


def test_reference_state_dict_replaces_exactly_the_llm_matrices():
    for cfg in (C.tiny(), C.tiny_2_5()):
        sd = random_state_dict(cfg, 0, "cpu")
        ref = fp4_reference_state_dict(sd, cfg)
        mats = {f"{L_PREFIX}layers.{i}.{m}.weight" for i in range(cfg.text.num_layers) for m in LLM_FP8_MATRICES}
        assert set(ref) == set(sd) | {"lm_head.weight"}, "tied embeddings: an explicit lm_head is added, nothing else"
        for k, v in ref.items():
            if k in mats:
                assert v.dtype == BF16 and v.shape == sd[k].shape
                assert torch.equal(v, dequantize_blocks_mxfp4(*quantize_blocks_mxfp4(sd[k]))) and not torch.equal(v, sd[k]), k
            elif k == "lm_head.weight":
                src = sd[k] if k in sd else sd[L_PREFIX + "embed_tokens.weight"]
                assert torch.equal(v, dequantize_rows_fp8(*quantize_rows_fp8_pow2(src))), "the head is e4m3 W'"
            else:
                assert v is sd[k], f"{k} must stay untouched"


def _model(cfg, sd, ops, **kw):
    return S.StreamingQwen2VL(cfg, sd, "cpu", ops=ops, max_len=1024, max_new_tokens=8, use_graph=False, **kw)


def untied(cfg):
    cfg = copy.deepcopy(cfg)
    cfg.text.tie_word_embeddings = False
    return cfg


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_fp4_engine_is_the_bf16_engine_on_the_dequantised_weights(family):
    """StreamingQwen2VL(sd, llm_fp4=True) on the CPU reference of the fp4 ops == StreamingQwen2VL(fp4_reference_state_dict(sd)) in bf16:
    identical eviction traces, KV lengths, tokens and every forward's logits, bit for bit."""
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    sdp = fp4_reference_state_dict(sd, cfg)
    kw = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8) if family == "qwen2_5" else {}
    outs = []
    for model in (_model(cfg, sd, RefOpsFp4(), llm_fp4=True), _model(untied(cfg), sdp, RefOps())):
        res, trace, counts, log = H.run_engine_stream(model, 4, keep_logits=True, **kw)
        outs.append((trace, [e["ids"] for e in log], [e["kv_len"] for e in log], [torch.stack(e["logits"]) for e in log]))
    assert outs[0][:3] == outs[1][:3]
    for a, b in zip(outs[0][3], outs[1][3]):
        assert torch.equal(a, b)
    plain = H.run_engine_stream(_model(cfg, sd, RefOps()), 1, keep_logits=True)[3]
    assert not torch.equal(torch.stack(plain[0]["logits"]), outs[0][3][0][:len(plain[0]["logits"])])


def test_fp4_engine_keeps_fp4_weights_and_reports_their_bytes():
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    eng = _model(cfg, sd, RefOpsFp4(), llm_fp4=True)._svlm_engine
    tc, l4 = cfg.text, eng.w.layers[0]
    assert eng.llm_fp4 and not eng.llm_fp8 and l4["flat4"].dtype == torch.uint8 and not {"flat", "flat8", "qkv_w", "qkv_w8"} & set(l4)
    assert eng.w.lm_head is None and eng.w.lm_head8.dtype == torch.float8_e4m3fn and eng.w.embed.dtype == BF16
    H_, I, qd, kd = tc.hidden_size, tc.intermediate_size, tc.num_heads * tc.head_dim, tc.num_kv_heads * tc.head_dim
    shapes = dict(qkv_w=(qd + 2 * kd, H_), o_w=(H_, qd), gu_w=(2 * I, H_), down_w=(H_, I))
    want = 0
    for name, (N, K) in shapes.items():
        assert l4[name + "4"].shape == (N, K // 2) and l4[name + "_s4"].shape == (N, K // 32)
        want += N * K // 2 + N * K // 32
    assert l4["flat4"].numel() + l4["scale4"].numel() == want
    want = tc.num_layers * (want + 2 * 2 * H_ + 2 * (qd + 2 * kd)) + 2 * H_ + tc.vocab_size * H_ + 4 * tc.vocab_size
    assert eng.w.decode_weight_bytes() == eng.w.decode_bytes() == want
    # the views are the quantiser's output, matrix by matrix
    p = f"{L_PREFIX}layers.0."
    codes, scales = quantize_blocks_mxfp4(sd[p + "self_attn.o_proj.weight"])
    assert torch.equal(l4["o_w4"], codes) and torch.equal(l4["o_w_s4"], scales)


def test_fp4_engine_refusals():
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    with pytest.raises(ValueError, match="llm_fp8"):
        _model(cfg, sd, RefOpsFp4(), llm_fp4=True, llm_fp8=True)
    with pytest.raises(ValueError, match="decode_tail"):
        _model(cfg, sd, RefOpsFp4(), llm_fp4=True, decode_tail=True)
    with pytest.raises(ValueError, match="prefill_fp8"):
        _model(cfg, sd, RefOpsFp4(), llm_fp4=True, prefill_fp8=True)
    with pytest.raises(ValueError, match="fp4 entry points"):
        _model(cfg, sd, RefOpsFp8(), llm_fp4=True)
    odd = C.tiny()
    odd.text.intermediate_size = 528          # a multiple of 16 (llm_fp8 takes it), not of 32
    with pytest.raises(ValueError, match="multiple of 32"):
        _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsFp4(), llm_fp4=True)
    base = _model(cfg, sd, RefOpsFp4(), llm_fp4=True)._svlm_engine
    with pytest.raises(ValueError, match="llm_fp4"):
        SvlmEngine(cfg, None, "cpu", share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    with pytest.raises(ValueError, match="llm_fp4"):
        SvlmEngine(cfg, None, "cpu", llm_fp8=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    lane = SvlmEngine(cfg, None, "cpu", llm_fp4=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    assert lane.w is base.w and lane._fp8_scratch_owner is base
    with pytest.raises(ValueError, match="llm_fp4"):
        StreamGroup(base, 2)
    assert not _model(cfg, sd, RefOps())._svlm_engine.llm_fp4          # the bf16 default needs none of it


def test_shared_fp4_engines_prefill_through_one_scratch_layer():
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    model = _model(cfg, sd, RefOpsFp4(), llm_fp4=True)
    base = model._svlm_engine
    assert base._fp8_scratch is None, "the scratch layer is allocated by the first prefill"
    want = H.run_engine_stream(model, 2, keep_logits=True)
    assert base._fp8_scratch is not None and base._fp8_scratch["gu_w"].dtype == BF16
    lane = SimpleNamespace(_svlm_engine=SvlmEngine(cfg, None, "cpu", llm_fp4=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False),
                           config=cfg, device=torch.device("cpu"))
    assert lane._svlm_engine._fp8_scratch is None
    lane._svlm_engine._dequant_layer(base.w.layers[1])
    assert lane._svlm_engine._fp8_scratch is base._fp8_scratch
    l1 = base.w.layers[1]
    assert torch.equal(base._fp8_scratch["down_w"], dequantize_blocks_mxfp4(l1["down_w4"], l1["down_w_s4"]))
    assert want[1]                                      # the stream generated tokens
