"""`SvlmEngine(llm_fp4=True, prefill_fp4=True)` on the MI355X, end to end: the prefill reads the MXFP4 weights itself
(csrc/gemm_wfp4.hip).  Two yardsticks: the oracle on W' = fp4_reference_state_dict(W) at the bars of every bf16 stream
(tests/test_engine_gpu.py:_compare: exact greedy tokens), and the scratch-layer `llm_fp4=True` engine of the same weights.  The direct
GEMMs feed their MFMAs the operands the scratch layer holds, under the same plan, so every forward's logits must be EQUAL to the
scratch engine's bit for bit, with equal tokens, token counts, eviction traces and KV lengths."""
import pytest
import torch

import helpers as H
from test_engine_gpu import _compare
from test_llm_fp4_gpu import untied

pytestmark = pytest.mark.gpu


def _pair(cfg, sd, **kw):
    """(direct, scratch) models of one set of weights."""
    import streaming_vlm_amd as S
    dev = {k: v.cuda() for k, v in sd.items()}
    direct = S.StreamingQwen2VL(cfg, dev, "cuda", llm_fp4=True, prefill_fp4=True, **kw)
    scratch = S.StreamingQwen2VL(cfg, dev, "cuda", llm_fp4=True, **kw)
    assert direct._svlm_engine.prefill_fp4 and not scratch._svlm_engine.prefill_fp4
    return direct, scratch


def _same_streams(direct, scratch, n_chunks, what, scratch_used=False, **kw):
    a = H.run_engine_stream(direct, n_chunks, keep_logits=True, **kw)
    b = H.run_engine_stream(scratch, n_chunks, keep_logits=True, **kw)
    assert a[1] == b[1], f"{what}: eviction traces differ"
    assert a[2] == b[2], f"{what}: token counts differ"
    n_tok = n_equal = 0
    for x, y in zip(a[3], b[3]):
        assert x["ids"] == y["ids"] and x["new"] == y["new"] and x["kv_len"] == y["kv_len"], what
        for u, v in zip(x["logits"], y["logits"]):
            n_equal += int(torch.equal(u, v))
            n_tok += 1
    print(f"[prefill_fp4 {what}] {n_tok} forwards, tokens / traces / KV lengths equal; {n_equal} of {n_tok} logit vectors bit-equal to the "
          f"scratch path")
    assert n_tok > 0 and n_equal == n_tok, f"{what}: {n_tok - n_equal} of {n_tok} forwards differ from the scratch engine"
    assert (direct._svlm_engine._fp8_scratch is not None) == scratch_used and scratch._svlm_engine._fp8_scratch is not None
    return a


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_tiny_streams_equal_the_oracle_tokens_and_the_scratch_engine_bits(family):
    """Graph replay on (the default), sink + window eviction (qwen2) and the structural policy (qwen2_5)."""
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import fp4_reference_state_dict
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    direct, scratch = _pair(cfg, sd, max_len=768, max_new_tokens=8)
    assert direct._svlm_engine.use_graph
    kw = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8,
              previous_text="a b c d e f g h i j k l m n o p") if family == "qwen2_5" else {}
    out = _compare(untied(cfg), fp4_reference_state_dict(sd, cfg), 7, direct, **kw)
    assert out["same"] == out["steps"]
    assert direct._svlm_engine._fp8_scratch is None
    a = _same_streams(direct, scratch, 7, f"tiny {family}", **kw)
    assert sum(1 for t in a[1] if t) >= 1, "the stream must evict for this test to mean anything"


def test_7b_width_stream_runs_the_590_row_shapes():
    """Qwen2-VL-7B widths, 2 LLM layers / 1 ViT block, 448 x 448 at 4 frames per second: two temporal grids per chunk, M ~ 590 prefills
    (qkv 4608 x 3584, o_proj 3584 x 3584 split 2 with the norm in the reduce, gate/up SwiGLU 18944 x 3584 on 128-row tiles, down_proj
    3584 x 18944 split 3)."""
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    cfg = C.qwen2_vl_7b()
    cfg.text.num_layers, cfg.vision.depth = 2, 1
    sd = random_state_dict(cfg, 0, "cpu")
    direct, scratch = _pair(cfg, sd, max_len=4608, max_new_tokens=4)
    rows = []
    o = direct._svlm_engine.ops
    inner = o.gemm_wfp4

    def spy(A, *a, **k):
        rows.append(int(A.shape[0]))
        return inner(A, *a, **k)
    o.gemm_wfp4 = spy
    try:
        _same_streams(direct, scratch, 2, "7B widths", size=448, fps=4.0, window=4096, max_new=4)
    finally:
        del o.gemm_wfp4
    assert rows and all(520 <= m <= 640 for m in rows), rows


def test_passes_above_the_row_threshold_use_the_scratch_layer_and_give_the_same_bits():
    """`PREFILL_FP4_MAX_ROWS` lowered on the instance: every prefill of the tiny stream goes through `_dequant_layer`."""
    from streaming_vlm_amd import config as C
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    direct, scratch = _pair(cfg, sd, max_len=768, max_new_tokens=8)
    direct._svlm_engine.PREFILL_FP4_MAX_ROWS = 8
    calls = []
    o = direct._svlm_engine.ops
    inner = o.gemm_wfp4

    def spy(*a, **k):
        calls.append(1)
        return inner(*a, **k)
    o.gemm_wfp4 = spy
    try:
        _same_streams(direct, scratch, 4, "threshold 8 rows", scratch_used=True)
    finally:
        del o.gemm_wfp4
    assert not calls, "a pass above the threshold took the direct GEMMs"
