"""Opt-in fp8 language-model weights, host side (no GPU): the power-of-two row quantiser, the bf16 reference image W' of an fp8
model, and the engine's sequencing of the fp8 decode step and dequantising prefill on the CPU reference backend -- which must be
the bf16 engine on W', bit for bit."""
import copy

import pytest
import torch

import helpers as H
from ref_ops import RefOps
from ref_ops_fp8 import RefOpsFp8

import streaming_vlm_amd as S
from streaming_vlm_amd import config as C
from streaming_vlm_amd.weights import (L_PREFIX, LLM_FP8_MATRICES, dequantize_rows_fp8, fp8_reference_state_dict, quantize_rows_fp8_pow2,
                                       random_state_dict)


def _w(shape=(512, 384), seed=0, std=0.02):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * std).to(torch.bfloat16)


def test_quantiser_scales_are_powers_of_two_and_codes_never_saturate():
    w = _w()
    w[7] *= 1000.0                  # one loud row, its own scale
    q, s = quantize_rows_fp8_pow2(w)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.float32 and q.shape == w.shape and s.shape == (w.shape[0],)
    m, _ = torch.frexp(s)
    assert bool((m == 0.5).all()), "every scale is an exact power of two"
    assert float(q.float().abs().max()) <= 448.0 and bool(torch.isfinite(q.float()).all())
    # the smallest power of two with amax / s <= 448: halving it would saturate
    amax = w.float().abs().amax(1)
    assert bool((amax <= 448.0 * s).all()) and bool((amax > 448.0 * s / 2).all())


def test_dequantised_weights_round_trip_through_bf16_bit_for_bit():
    for seed, std in ((0, 0.02), (1, 3.0), (2, 1e-5)):
        q, s = quantize_rows_fp8_pow2(_w((256, 1536), seed, std))
        wf = q.float() * s.unsqueeze(1)
        assert torch.equal(wf.to(torch.bfloat16).float(), wf)
        assert torch.equal(dequantize_rows_fp8(q, s).float(), wf)
        # the fp8 GEMV (scale once, after the sum) is the bf16 GEMV on W' up to the summation order: here the same order, same bits
        x = torch.randn(1536, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16).float()
        assert torch.equal((q.float() @ x) * s, wf @ x)


def test_zero_rows_get_scale_one_and_exact_power_of_two_ratios_keep_their_scale():
    w = _w((8, 64))
    w[2] = 0
    w[5] = 0
    w[5, 3] = -448.0 * 2.0 ** -10            # amax / 448 = 2^-10 exactly
    w[6] = 0
    w[6, 0] = 448.0 * 2.0 ** -10 * 1.0078125  # one bf16 step above: the next power
    q, s = quantize_rows_fp8_pow2(w)
    assert float(s[2]) == 1.0 and bool((q[2].float() == 0).all())
    assert float(s[5]) == 2.0 ** -10 and float(q[5, 3].float()) == -448.0
    assert float(s[6]) == 2.0 ** -9


def test_reference_state_dict_replaces_exactly_the_llm_matrices():
    for cfg in (C.tiny(), C.tiny_2_5()):
        sd = random_state_dict(cfg, 0, "cpu")
        ref = fp8_reference_state_dict(sd, cfg)
        want = {f"{L_PREFIX}layers.{i}.{m}.weight" for i in range(cfg.text.num_layers) for m in LLM_FP8_MATRICES} | {"lm_head.weight"}
        assert set(ref) == set(sd) | {"lm_head.weight"}, "tied embeddings: an explicit lm_head is added, nothing else"
        for k, v in ref.items():
            if k in want:
                assert v.dtype == torch.bfloat16 and v.shape == (sd[k] if k in sd else sd[L_PREFIX + "embed_tokens.weight"]).shape
                src = sd[k] if k in sd else sd[L_PREFIX + "embed_tokens.weight"]
                assert torch.equal(v, dequantize_rows_fp8(*quantize_rows_fp8_pow2(src))), k
                assert not torch.equal(v, src), k
            else:
                assert v is sd[k], f"{k} must stay untouched"


def _model(cfg, sd, ops, **kw):
    return S.StreamingQwen2VL(cfg, sd, "cpu", ops=ops, max_len=1024, max_new_tokens=8, use_graph=False, **kw)


def untied(cfg):
    """The bf16 model of fp8_reference_state_dict(sd): its explicit lm_head.weight (W' of the embedding when the embeddings are tied)
    is a matrix of its own, so the engine must read it as an untied model does (the oracle prefers it whenever it is present)."""
    cfg = copy.deepcopy(cfg)
    cfg.text.tie_word_embeddings = False
    return cfg


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_fp8_engine_is_the_bf16_engine_on_the_dequantised_weights(family):
    """StreamingQwen2VL(sd, llm_fp8=True) on the CPU reference of the fp8 ops == StreamingQwen2VL(fp8_reference_state_dict(sd)) in bf16:
    identical eviction traces, KV lengths, tokens and every forward's logits, bit for bit (prefill through the scratch layer, decode
    steps and prefill logits through the fp8 GEMVs)."""
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    sdp = fp8_reference_state_dict(sd, cfg)
    kw = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8) if family == "qwen2_5" else {}
    outs = []
    for model in (_model(cfg, sd, RefOpsFp8(), llm_fp8=True), _model(untied(cfg), sdp, RefOps())):
        res, trace, counts, log = H.run_engine_stream(model, 4, keep_logits=True, **kw)
        outs.append((trace, [e["ids"] for e in log], [e["kv_len"] for e in log], [torch.stack(e["logits"]) for e in log]))
    assert outs[0][:3] == outs[1][:3]
    for a, b in zip(outs[0][3], outs[1][3]):
        assert torch.equal(a, b)
    # ... and it is a different model from the bf16 one on W
    plain = H.run_engine_stream(_model(cfg, sd, RefOps()), 1, keep_logits=True)[3]
    assert not torch.equal(torch.stack(plain[0]["logits"]), outs[0][3][0][:len(plain[0]["logits"])])


def test_fp8_engine_keeps_fp8_weights_and_reports_their_bytes():
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    e8 = _model(cfg, sd, RefOpsFp8(), llm_fp8=True)._svlm_engine
    e16 = _model(cfg, sd, RefOps())._svlm_engine
    l8 = e8.w.layers[0]
    assert l8["flat8"].dtype == torch.float8_e4m3fn and "flat" not in l8 and "qkv_w" not in l8
    assert e8.w.lm_head is None and e8.w.lm_head8.dtype == torch.float8_e4m3fn and e8.w.embed.dtype == torch.bfloat16
    tc = cfg.text
    n_layer = sum(l8[k].numel() for k in ("qkv_w8", "o_w8", "gu_w8", "down_w8"))
    n_rows = sum(l8[k].numel() for k in ("qkv_w_s", "o_w_s", "gu_w_s", "down_w_s"))
    assert n_layer == e16.w.layers[0]["flat"].numel() and n_rows == l8["scale"].numel()
    assert e16.w.decode_bytes() - e8.w.decode_bytes() == tc.num_layers * (n_layer - 4 * n_rows) + tc.vocab_size * tc.hidden_size - 4 * tc.vocab_size
    assert e16.w.nbytes_llm_decode() == e16.w.decode_bytes()


def test_fp8_engine_refusals():
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    with pytest.raises(ValueError, match="decode_tail"):
        _model(cfg, sd, RefOpsFp8(), llm_fp8=True, decode_tail=True)
    with pytest.raises(ValueError, match="fp8 entry points"):
        _model(cfg, sd, RefOps(), llm_fp8=True)
    odd = C.tiny()
    odd.text.intermediate_size = 520          # a multiple of 8, not of 16
    with pytest.raises(ValueError, match="multiple of 16"):
        _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsFp8(), llm_fp8=True)
    # the bf16 default needs none of it
    assert not _model(cfg, sd, RefOps())._svlm_engine.llm_fp8
