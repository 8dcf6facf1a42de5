"""Stream groups on fp8 language-model weights, end to end.  Yardstick: the same stream run ALONE on the same llm_fp8=True model through
streaming_inference; per lane the responses, token counts, cache lengths, eviction traces and logical id order must be EXACTLY equal
(the lane-batched fp8 kernels are bitwise the single-row fp8 ones per lane, tests/test_decode_batch_fp8_gpu.py)."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu


def _fp8_model(family="qwen2", use_graph=True, max_new=8, stream=None, cfg=None, max_len=768):
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    if cfg is None:
        cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg, **(stream or dict(max_new=max_new)))
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=max_len, max_new_tokens=max_new, use_graph=use_graph,
                               llm_fp8=True)
    assert model._svlm_engine.llm_fp8
    return cfg, model


def _stream_kw(cfg, size, n_chunks, previous_text, query, max_new=8, suppress_eos=True, window=64, fps=1.0):
    size_s = f"{size[1]}x{size[0]}" if isinstance(size, (tuple, list)) else f"{size}x{size}"
    return dict(video_path=f"synthetic://{size_s}@{fps:g}fps", model_base="Qwen2_5" if cfg.family == "qwen2_5" else "Qwen2", duration=n_chunks,
                previous_text=previous_text, query=query, kv_policy="sink_window", sink=4, window=window, do_sample=False,
                max_new_tokens=max_new, suppress_eos=suppress_eos, quiet=True)


def _run(fn, kw):
    """One stream with its logs: (responses, eviction trace, token counts, [(ids, kv_len)] per chunk)."""
    logs = dict(trace=[], token_counts=[], ids_log=[])
    res = fn(dict(kw, **logs))
    return res, logs


def _same_stream(i, got, want):
    (gr, gl), (wr, wl) = got, want
    assert [r["response"] for r in gr] == [r["response"] for r in wr], f"stream {i}: responses differ"
    assert gl["trace"] == wl["trace"], f"stream {i}: eviction traces differ"
    assert gl["token_counts"] == wl["token_counts"], f"stream {i}: n_new per chunk differs"
    assert len(gl["ids_log"]) == len(wl["ids_log"])
    for c, (a, b) in enumerate(zip(gl["ids_log"], wl["ids_log"])):
        assert a["ids"] == b["ids"] and a["new"] == b["new"], f"stream {i} chunk {c}: logical id order / new tokens differ"
        assert a["kv_len"] == b["kv_len"], f"stream {i} chunk {c}: cache length differs"


def _solo_and_group(cfg, model, streams, n_lanes):
    import streaming_vlm_amd as S
    proc = S.SyntheticProcessor()
    solo = [_run(lambda kw: S.streaming_inference(model=model, processor=proc, **kw), s) for s in streams]
    logs = [dict(trace=[], token_counts=[], ids_log=[]) for _ in streams]
    res = S.streaming_inference_group(model, proc, [dict(s, **lg) for s, lg in zip(streams, logs)], n_lanes=n_lanes)
    return solo, list(zip(res, logs))


@pytest.mark.parametrize("use_graph", [True, False])
@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_three_fp8_streams_in_lock_step_equal_their_solo_runs(family, use_graph):
    """Different prompts, frame sizes and chunk counts (the second ends four chunks before the others); the window makes every stream
    evict at least twice."""
    cfg, model = _fp8_model(family, use_graph, stream=dict(size=(112, 84)))
    streams = [_stream_kw(cfg, 56, 9, "hello world", "Commentate on this match"),
               _stream_kw(cfg, (112, 84), 5, "the game begins", "What happens now", window=96),
               _stream_kw(cfg, 84, 9, "", "Describe the scene")]
    solo, grouped = _solo_and_group(cfg, model, streams, 3)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        assert sum(1 for t in w[1]["trace"] if t) >= 2, f"stream {i} must evict at least twice for this test to mean anything: {w[1]['trace']}"
        _same_stream(i, g, w)


def test_2b_width_four_fp8_lanes_three_chunks():
    """Real Qwen2-VL-2B widths (4 LLM layers / 4 ViT blocks), B = 4, exact tokens."""
    from streaming_vlm_amd import config as C
    cfg = C.qwen2_vl_2b()
    cfg.vision.depth = 4
    cfg.text.num_layers = 4
    cfg, model = _fp8_model(cfg=cfg, stream=dict(size=224), max_len=1024)
    streams = [_stream_kw(cfg, 224, 3, t, q, window=128) for t, q in (("hello world", "Commentate on this match"), ("the game begins", "What happens now"),
                                                                      ("one two three", "Describe the scene"), ("", "Commentate on this match"))]
    solo, grouped = _solo_and_group(cfg, model, streams, 4)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def _weight_tensors(w):
    """Every weight tensor of an llm_fp8 engine: bf16 ones, the e4m3 codes (`*8`, `flat8`) and the row scales (`*_s`, `scale`)."""
    out = dict(embed=w.embed, lm_head8=w.lm_head8, lm_head_s=w.lm_head_s, final_norm=w.final_norm, patch_embed=w.patch_embed)
    for name, blocks in (("layer", w.layers), ("vit", w.vit)):
        for bi, blk in enumerate(blocks):
            out.update({f"{name}{bi}.{k}": v for k, v in blk.items() if torch.is_tensor(v)})
    out.update({f"merger.{k}": v for k, v in w.merger.items() if torch.is_tensor(v)})
    return out


def test_fp8_weights_and_the_prefill_scratch_layer_are_shared():
    """No second copy of any weight tensor, codes and scales included, and ONE bf16 scratch layer for the prefills of all lanes."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model = _fp8_model("qwen2", True)
    eng = model._svlm_engine
    before = torch.cuda.memory_allocated()
    group = StreamGroup(eng, 3)
    grown = torch.cuda.memory_allocated() - before
    base = _weight_tensors(eng.w)
    assert any(k.endswith("qkv_w8") for k in base) and any(k.endswith("down_w_s") for k in base)
    weight_bytes = sum(t.numel() * t.element_size() for t in {t.data_ptr(): t for t in base.values()}.values())
    for lane in group.lanes:
        assert lane.llm_fp8
        mine = _weight_tensors(lane.w)
        assert mine.keys() == base.keys()
        for k in base:
            assert mine[k].data_ptr() == base[k].data_ptr(), k
        assert lane.inv_freq.data_ptr() == eng.inv_freq.data_ptr()
    # two extra lanes: per-stream buffers only (no KV pool yet) -- well below one copy of the weights per lane
    assert grown / 2 < 0.25 * weight_bytes, (grown, weight_bytes)
    # every lane prefills once (one chunk through the group), then: one scratch layer
    proc = S.SyntheticProcessor()
    srcs = [H.chunk_source(proc, S.SyntheticVideo(56, 1.0, 0), t) for t in ("hello world", "the game begins", "a b c")]
    reqs = []
    for src in srcs:
        ids, pix, grid = src(0)
        reqs.append(dict(ids=ids, cache=None, video_grid_thw=grid, pixel_values=pix.cuda(), grid_thw=grid, max_new_tokens=4, do_sample=False,
                         suppress_eos=True))
    want = [eng.generate(**dict(r)) for r in reqs]
    got = group.generate(reqs)
    for g, w in zip(got, want):
        assert g.sequences == w.sequences and g.n_new == w.n_new == 4
    scratch = [lane._fp8_scratch for lane in group.lanes]
    assert all(sc is not None for sc in scratch)
    for sc in scratch:
        for name in ("qkv_w", "o_w", "gu_w", "down_w"):
            assert sc[name].data_ptr() == scratch[0][name].data_ptr(), f"a lane dequantises {name} into a scratch layer of its own"
        assert sc["qkv_w"].untyped_storage().data_ptr() == scratch[0]["down_w"].untyped_storage().data_ptr()


def test_refused_configurations_of_an_fp8_group():
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model = _fp8_model("qwen2", True)
    group = StreamGroup(model._svlm_engine, 2)
    req = dict(ids=[1, 2, 3], cache=None, video_grid_thw=[], max_new_tokens=4)
    for extra in (dict(do_sample=True), dict(do_sample=True, top_k=5), dict(force_tokens=[1]), dict(keep_logits=True)):
        with pytest.raises(ValueError, match="stream group"):
            group.generate([dict(req, **extra), None])
    eng = model._svlm_engine
    eng.decode_tail = True                   # (an fp8 engine cannot be built with the tail; the group's own refusal is what is checked)
    try:
        with pytest.raises(ValueError, match="stream group"):
            StreamGroup(eng, 2)
    finally:
        eng.decode_tail = False
