"""`SvlmEngine(llm_fp8=True, prefill_fp8=True)` on the MI355X, end to end: the prefill reads the e4m3 weights itself (csrc/gemm_wfp8.hip).
Yardstick: the scratch-layer `llm_fp8=True` engine of the same weights, which is held to the oracle on W' by tests/test_llm_fp8_gpu.py.
Both feed their MFMAs the same operands, so greedy tokens, token counts, eviction traces and KV lengths must be EXACTLY equal; logits
are compared as tests/test_llm_fp8_gpu.py compares two engines of one model (mean rel <= 5e-3, max rel <= 5e-2), and printed."""
import pytest
import torch

import helpers as H
from test_engine_gpu import _rel
from test_stream_group_fp8_gpu import _run, _same_stream, _stream_kw

pytestmark = pytest.mark.gpu


def _pair(cfg, sd, **kw):
    """(direct, scratch) models of one set of weights."""
    import streaming_vlm_amd as S
    dev = {k: v.cuda() for k, v in sd.items()}
    direct = S.StreamingQwen2VL(cfg, dev, "cuda", llm_fp8=True, prefill_fp8=True, **kw)
    scratch = S.StreamingQwen2VL(cfg, dev, "cuda", llm_fp8=True, **kw)
    assert direct._svlm_engine.prefill_fp8 and not scratch._svlm_engine.prefill_fp8
    return direct, scratch


def _same_streams(direct, scratch, n_chunks, what, **kw):
    a = H.run_engine_stream(direct, n_chunks, keep_logits=True, **kw)
    b = H.run_engine_stream(scratch, n_chunks, keep_logits=True, **kw)
    assert a[1] == b[1], f"{what}: eviction traces differ"
    assert a[2] == b[2], f"{what}: token counts differ"
    worst_max = worst_mean = 0.0
    n_tok = n_equal = 0
    for x, y in zip(a[3], b[3]):
        assert x["ids"] == y["ids"] and x["new"] == y["new"] and x["kv_len"] == y["kv_len"], what
        for u, v in zip(x["logits"], y["logits"]):
            mx, mn = _rel(u, v)
            worst_max, worst_mean = max(worst_max, mx), max(worst_mean, mn)
            n_equal += int(torch.equal(u, v))
            n_tok += 1
    print(f"[prefill_fp8 {what}] {n_tok} forwards, tokens / traces / KV lengths equal; logits vs the scratch path: max rel {worst_max:.3e} "
          f"mean rel {worst_mean:.3e}, {n_equal} of {n_tok} bit-equal")
    assert worst_mean <= 5e-3 and worst_max <= 5e-2
    assert direct._svlm_engine._fp8_scratch is None and scratch._svlm_engine._fp8_scratch is not None
    return a


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_tiny_streams_equal_the_scratch_engine(family):
    """Graph replay on (the default), sink + window eviction (qwen2) and the structural policy (qwen2_5)."""
    from streaming_vlm_amd import config as C
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    direct, scratch = _pair(cfg, sd, max_len=768, max_new_tokens=8)
    assert direct._svlm_engine.use_graph
    kw = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8,
              previous_text="a b c d e f g h i j k l m n o p") if family == "qwen2_5" else {}
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
    inner = o.gemm_wfp8

    def spy(A, *a, **k):
        rows.append(int(A.shape[0]))
        return inner(A, *a, **k)
    o.gemm_wfp8 = spy
    try:
        _same_streams(direct, scratch, 2, "7B widths", size=448, fps=4.0, window=4096, max_new=4)
    finally:
        del o.gemm_wfp8
    assert rows and all(520 <= m <= 640 for m in rows), rows


def test_three_lane_group_on_a_prefill_fp8_engine():
    """Each lane's stream equals its solo run on the same engine, and no lane ever has a scratch layer."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg = C.tiny()
    sd = H.decisive_weights(cfg, size=(112, 84))
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8, llm_fp8=True, prefill_fp8=True)
    streams = [_stream_kw(cfg, 56, 6, "hello world", "Commentate on this match"),
               _stream_kw(cfg, (112, 84), 4, "the game begins", "What happens now", window=96),
               _stream_kw(cfg, 84, 6, "", "Describe the scene")]
    proc = S.SyntheticProcessor()
    solo = [_run(lambda kw: S.streaming_inference(model=model, processor=proc, **kw), s) for s in streams]
    group = StreamGroup(model._svlm_engine, 3)
    assert all(ln.prefill_fp8 for ln in group.lanes)
    logs = [dict(trace=[], token_counts=[], ids_log=[]) for _ in streams]
    res = S.streaming_inference_group(model, proc, [dict(s, **lg) for s, lg in zip(streams, logs)], group=group)
    for i, (g, w) in enumerate(zip(zip(res, logs), solo)):
        _same_stream(i, g, w)
    assert all(ln._fp8_scratch is None for ln in group.lanes) and model._svlm_engine._fp8_scratch_owner._fp8_scratch is None
