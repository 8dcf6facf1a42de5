"""Stream groups on MXFP4 language-model weights, end to end.  Yardstick: the same stream run ALONE on the same llm_fp4=True model
through streaming_inference; per lane the responses, token counts, cache lengths, eviction traces and logical id order must be EXACTLY
equal (the lane-batched fp4 kernels are bitwise the single-row fp4 ones per lane, tests/test_decode_batch_fp4_gpu.py)."""
import pytest
import torch

import helpers as H
from test_stream_group_fp8_gpu import _same_stream, _solo_and_group, _stream_kw

pytestmark = pytest.mark.gpu


def _fp4_model(family="qwen2", use_graph=True, max_new=8, stream=None, cfg=None, max_len=768, prefill_fp4=False):
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    if cfg is None:
        cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg, **(stream or dict(max_new=max_new)))
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=max_len, max_new_tokens=max_new, use_graph=use_graph,
                               llm_fp4=True, prefill_fp4=prefill_fp4)
    assert model._svlm_engine.llm_fp4 and model._svlm_engine.prefill_fp4 == prefill_fp4 and not model._svlm_engine.llm_fp8
    return cfg, model


@pytest.mark.parametrize("prefill_fp4", [False, True], ids=["scratch", "prefill_fp4"])
@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_three_fp4_streams_in_lock_step_equal_their_solo_runs(family, use_graph, prefill_fp4):
    """Different prompts, frame sizes and chunk counts (the second ends four chunks before the others); the window makes every stream
    evict at least twice."""
    cfg, model = _fp4_model(family, use_graph, stream=dict(size=(112, 84)), prefill_fp4=prefill_fp4)
    streams = [_stream_kw(cfg, 56, 9, "hello world", "Commentate on this match"),
               _stream_kw(cfg, (112, 84), 5, "the game begins", "What happens now", window=96),
               _stream_kw(cfg, 84, 9, "", "Describe the scene")]
    solo, grouped = _solo_and_group(cfg, model, streams, 3)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        assert sum(1 for t in w[1]["trace"] if t) >= 2, f"stream {i} must evict at least twice for this test to mean anything: {w[1]['trace']}"
        _same_stream(i, g, w)


def test_2b_width_four_fp4_lanes_three_chunks():
    """Real Qwen2-VL-2B widths (4 LLM layers / 4 ViT blocks), B = 4, the direct MXFP4 prefill, exact tokens."""
    from streaming_vlm_amd import config as C
    cfg = C.qwen2_vl_2b()
    cfg.vision.depth = 4
    cfg.text.num_layers = 4
    cfg, model = _fp4_model(cfg=cfg, stream=dict(size=224), max_len=1024, prefill_fp4=True)
    streams = [_stream_kw(cfg, 224, 3, t, q, window=128) for t, q in (("hello world", "Commentate on this match"), ("the game begins", "What happens now"),
                                                                      ("one two three", "Describe the scene"), ("", "Commentate on this match"))]
    solo, grouped = _solo_and_group(cfg, model, streams, 4)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def _weight_tensors(w):
    """Every weight tensor of an llm_fp4 engine: bf16 ones, the e2m1 codes (`*4`, `flat4`), the e8m0 block scales (`*_s4`) and the e4m3
    head with its row scales."""
    out = dict(embed=w.embed, lm_head8=w.lm_head8, lm_head_s=w.lm_head_s, final_norm=w.final_norm, patch_embed=w.patch_embed)
    for name, blocks in (("layer", w.layers), ("vit", w.vit)):
        for bi, blk in enumerate(blocks):
            out.update({f"{name}{bi}.{k}": v for k, v in blk.items() if torch.is_tensor(v)})
    out.update({f"merger.{k}": v for k, v in w.merger.items() if torch.is_tensor(v)})
    return out


def _one_chunk_requests(n):
    import streaming_vlm_amd as S
    proc = S.SyntheticProcessor()
    srcs = [H.chunk_source(proc, S.SyntheticVideo(56, 1.0, 0), t) for t in ("hello world", "the game begins", "a b c")[:n]]
    reqs = []
    for src in srcs:
        ids, pix, grid = src(0)
        reqs.append(dict(ids=ids, cache=None, video_grid_thw=grid, pixel_values=pix.cuda(), grid_thw=grid, max_new_tokens=4, do_sample=False,
                         suppress_eos=True))
    return reqs


@pytest.mark.parametrize("prefill_fp4", [False, True], ids=["scratch", "prefill_fp4"])
def test_fp4_weights_and_the_prefill_scratch_layer_are_shared(prefill_fp4):
    """No second copy of any weight tensor, codes and block scales included; every lane carries the group engine's flags; on the scratch
    path ONE bf16 scratch layer serves the prefills of all lanes, on the direct path nobody allocates one."""
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model = _fp4_model("qwen2", True, prefill_fp4=prefill_fp4)
    eng = model._svlm_engine
    before = torch.cuda.memory_allocated()
    group = StreamGroup(eng, 3)
    grown = torch.cuda.memory_allocated() - before
    base = _weight_tensors(eng.w)
    assert any(k.endswith("qkv_w4") for k in base) and any(k.endswith("down_w_s4") for k in base) and any(k.endswith("gu_w_s4") for k in base)
    weight_bytes = sum(t.numel() * t.element_size() for t in {t.data_ptr(): t for t in base.values()}.values())
    for lane in group.lanes:
        assert lane.llm_fp4 and lane.prefill_fp4 == eng.prefill_fp4 == prefill_fp4 and not lane.llm_fp8
        mine = _weight_tensors(lane.w)
        assert mine.keys() == base.keys()
        for k in base:
            assert mine[k].data_ptr() == base[k].data_ptr(), k
        assert lane.inv_freq.data_ptr() == eng.inv_freq.data_ptr()
    # two extra lanes: per-stream buffers only (no KV pool yet) -- well below one copy of the weights per lane
    assert grown / 2 < 0.25 * weight_bytes, (grown, weight_bytes)
    # every lane prefills once (one chunk through the group)
    reqs = _one_chunk_requests(3)
    want = [eng.generate(**dict(r)) for r in reqs]
    got = group.generate(reqs)
    for g, w in zip(got, want):
        assert g.sequences == w.sequences and g.n_new == w.n_new == 4
    scratch = [lane._fp8_scratch for lane in group.lanes]
    if prefill_fp4:
        assert all(sc is None for sc in scratch), "a direct-prefill lane dequantised into a scratch layer"
        return
    assert all(sc is not None for sc in scratch)
    for sc in scratch:
        for name in ("qkv_w", "o_w", "gu_w", "down_w"):
            assert sc[name].data_ptr() == scratch[0][name].data_ptr(), f"a lane dequantises {name} into a scratch layer of its own"
        assert sc["qkv_w"].untyped_storage().data_ptr() == scratch[0]["down_w"].untyped_storage().data_ptr()


def test_one_sampled_batch_on_fp4_weights_mixes_greedy_temperature_and_top_k_top_p():
    """A greedy lane, a plain-temperature lane and a top-k / top-p lane in one batch of a sampling=True group: per lane the tokens of the
    stream run alone on a fresh engine with the same generator seed (the method of tests/test_stream_group_sampling_gpu.py)."""
    from streaming_vlm_amd import config as C
    from test_stream_group_sampling_gpu import _group, _solo, _stream_kw as _sampled_kw, _weights
    from test_stream_group_sampling_gpu import _same_stream as _same_sampled
    cfg = C.tiny()
    sd = _weights(cfg)
    streams = [_sampled_kw(cfg, 56, 3, "hello world", "Commentate on this match", None, None),
               _sampled_kw(cfg, 84, 3, "the game begins", "What happens now", (0.9, 0, 1.0), 7),
               _sampled_kw(cfg, 56, 3, "", "Describe the scene", (0.9, 50, 0.9), 5)]
    solo = [_solo(cfg, sd, s, llm_fp4=True, prefill_fp4=True) for s in streams]
    grouped = _group(cfg, sd, streams, llm_fp4=True, prefill_fp4=True)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_sampled(i, g, w)
    greedy = _solo(cfg, sd, dict(streams[1], do_sample=False, seed=None), llm_fp4=True, prefill_fp4=True)
    assert [r["response"] for r in greedy[0]] != [r["response"] for r in solo[1][0]], "T = 0.9 reproduced the argmax on these weights"


def test_refused_configurations_of_an_fp4_group():
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model = _fp4_model("qwen2", True)
    group = StreamGroup(model._svlm_engine, 2)
    req = dict(ids=[1, 2, 3], cache=None, video_grid_thw=[], max_new_tokens=4)
    for extra in (dict(do_sample=True), dict(do_sample=True, top_k=5), dict(force_tokens=[1]), dict(keep_logits=True)):
        with pytest.raises(ValueError, match="stream group"):
            group.generate([dict(req, **extra), None])
    eng = model._svlm_engine
    eng.decode_tail = True                   # (an fp4 engine cannot be built with the tail; the group's own refusal is what is checked)
    try:
        with pytest.raises(ValueError, match="stream group"):
            StreamGroup(eng, 2)
    finally:
        eng.decode_tail = False
