"""Stream groups end to end.  Yardstick: the same stream run ALONE through a plain SvlmEngine / streaming_inference built from the same
weights; per lane the tokens, token counts, cache lengths, eviction traces and logical id order must be EXACTLY equal."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu


def _model(family="qwen2", use_graph=True, max_new=8, stream=None, cfg=None, max_len=768):
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    if cfg is None:
        cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg, **(stream or dict(max_new=max_new)))
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=max_len, max_new_tokens=max_new, use_graph=use_graph)
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
def test_three_streams_in_lock_step_equal_their_solo_runs(family, use_graph):
    """Different prompts, frame sizes and chunk counts (the second ends four chunks before the others); the window makes every stream
    evict at least twice."""
    cfg, model = _model(family, use_graph, stream=dict(size=(112, 84)))
    streams = [_stream_kw(cfg, 56, 9, "hello world", "Commentate on this match"),
               _stream_kw(cfg, (112, 84), 5, "the game begins", "What happens now", window=96),
               _stream_kw(cfg, 84, 9, "", "Describe the scene")]
    solo, grouped = _solo_and_group(cfg, model, streams, 3)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        assert sum(1 for t in w[1]["trace"] if t) >= 2, f"stream {i} must evict at least twice for this test to mean anything: {w[1]['trace']}"
        _same_stream(i, g, w)


def test_eos_mid_chunk_different_max_new_tokens_and_weights_shared():
    """One lane meets EOS tokens mid-chunk (EOS not suppressed, copy-head weights: where it stops is known from its solo run) while the
    others run to their own, different, max_new_tokens."""
    from streaming_vlm_amd.stream_group import StreamGroup
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.config import IM_END
    from streaming_vlm_amd.weights import decisive_state_dict
    cfg = C.tiny()
    # the copy head repeats the token `offset` positions back: a short offset walks it over the prompt's closing <|im_end|> a few
    # steps into a chunk.  The first offset whose SOLO run stops mid-chunk (past the first EOS look at step 4) is the case.
    for offset in (10, 11, 9, 12, 8, 13, 14):
        sd = decisive_state_dict(cfg, 0, "cpu", offset=offset)
        # decisive_state_dict embeds the chat markers as half a stand-in token so that a copy never decodes to one; here <|im_end|>
        # gets an embedding of its own again, so the copy of the prompt's closing marker IS an end-of-turn token
        emb = next(v for k, v in sd.items() if k.endswith("embed_tokens.weight"))
        emb[IM_END] = (torch.randn(emb.shape[1], generator=torch.Generator().manual_seed(5)) * 0.02).to(emb.dtype)
        model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=16)
        streams = [_stream_kw(cfg, 56, 6, "hello world", "Commentate on this match", max_new=16, suppress_eos=False),
                   _stream_kw(cfg, 56, 6, "the game begins", "What happens now", max_new=5),
                   _stream_kw(cfg, 84, 6, "a b c", "Describe the scene", max_new=12)]
        counts = _run(lambda kw: S.streaming_inference(model=model, processor=S.SyntheticProcessor(), **kw), streams[0])[1]["token_counts"]
        print(f"copy offset {offset}: solo token counts of the EOS stream: {counts}")
        if any(4 < c < 16 for c in counts):
            break
    else:
        raise AssertionError("no copy offset makes the solo stream stop mid-chunk")
    solo, grouped = _solo_and_group(cfg, model, streams, 3)
    assert solo[0][1]["token_counts"] == counts
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)
    # no second copy of any weight tensor: every lane's weights ARE the group engine's
    eng = model._svlm_engine
    before = torch.cuda.memory_allocated()
    group = StreamGroup(eng, 3)
    grown = torch.cuda.memory_allocated() - before

    def tensors(w):
        out = dict(embed=w.embed, lm_head=w.lm_head, final_norm=w.final_norm, patch_embed=w.patch_embed)
        for name, blocks in (("layer", w.layers), ("vit", w.vit)):
            for bi, blk in enumerate(blocks):
                out.update({f"{name}{bi}.{k}": v for k, v in blk.items() if torch.is_tensor(v)})
        out.update({f"merger.{k}": v for k, v in w.merger.items() if torch.is_tensor(v)})
        return out

    base = tensors(eng.w)
    weight_bytes = sum(t.numel() * t.element_size() for t in {t.data_ptr(): t for t in base.values()}.values())
    for lane in group.lanes:
        mine = tensors(lane.w)
        assert mine.keys() == base.keys()
        for k in base:
            assert mine[k].data_ptr() == base[k].data_ptr(), k
        assert lane.inv_freq.data_ptr() == eng.inv_freq.data_ptr()
    # two extra lanes: per-stream buffers only (no KV pool yet) -- well below one copy of the weights per lane
    assert grown / 2 < 0.25 * weight_bytes, (grown, weight_bytes)


def test_generate_with_a_none_request_and_unequal_limits():
    """StreamGroup.generate directly: lane 1 has no request, lanes 0 and 2 stop at different max_new_tokens; graph replay twice."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model = _model("qwen2", True)
    eng = model._svlm_engine
    proc = S.SyntheticProcessor()
    srcs = [H.chunk_source(proc, S.SyntheticVideo(56, 1.0, 0), "hello world"), None,
            H.chunk_source(proc, S.SyntheticVideo(84, 1.0, 0), "the game begins", query="What happens now")]
    limits = [8, None, 3]
    group = StreamGroup(eng, 3)

    def reqs(cache_of, chunk):
        out = []
        for i, src in enumerate(srcs):
            if src is None:
                out.append(None)
                continue
            ids, pix, grid = src(chunk)
            c = cache_of[i]
            prev = cache_of.get(("ids", i), [])
            out.append(dict(ids=prev + ids, cache=c, video_grid_thw=cache_of.get(("g", i), []) + grid, pixel_values=pix.cuda(), grid_thw=grid,
                            max_new_tokens=limits[i], do_sample=False, suppress_eos=True))
        return out

    solo_state, grp_state = {0: None, 2: None}, {0: None, 1: None, 2: None}
    for chunk in range(2):
        want = {i: eng.generate(**r) for i, r in enumerate(reqs(solo_state, chunk)) if r is not None}
        got = group.generate(reqs(grp_state, chunk))
        assert got[1] is None
        for i in (0, 2):
            assert got[i].sequences == want[i].sequences and got[i].n_new == want[i].n_new == limits[i]
            assert got[i].past_key_values.length == want[i].past_key_values.length
            for st, o in ((solo_state, want[i]), (grp_state, got[i])):
                st[i] = o.past_key_values
                st[("ids", i)] = o.sequences
                st[("g", i)] = st.get(("g", i), []) + srcs[i](chunk)[2]


def test_four_streams_over_two_lanes_and_a_stream_that_raises():
    import streaming_vlm_amd as S
    cfg, model = _model("qwen2", True)
    streams = [_stream_kw(cfg, 56, 4, "hello world", "Commentate on this match"),
               _stream_kw(cfg, 84, 3, "the game begins", "What happens now"),
               _stream_kw(cfg, 56, 5, "one two three", "Describe the scene"),
               _stream_kw(cfg, 84, 2, "", "Commentate on this match")]
    solo, grouped = _solo_and_group(cfg, model, streams, 2)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)
    # stream 1 asks for more tokens than the engine was built for: it is reported with its index, the others complete
    bad = [dict(s) for s in streams]
    bad[1]["max_new_tokens"] = 99
    with pytest.raises(S.StreamGroupError) as ei:
        S.streaming_inference_group(model, S.SyntheticProcessor(), bad, n_lanes=2)
    assert ei.value.index == 1 and ei.value.results[1] is None and isinstance(ei.value.__cause__, ValueError)
    for i in (0, 2, 3):
        assert [r["response"] for r in ei.value.results[i]] == [r["response"] for r in solo[i][0]], i


def test_2b_width_four_lanes_three_chunks():
    """Real Qwen2-VL-2B widths (4 LLM layers / 4 ViT blocks, as test_engine_gpu.py does for width checks), B = 4, exact tokens."""
    from streaming_vlm_amd import config as C
    cfg = C.qwen2_vl_2b()
    cfg.vision.depth = 4
    cfg.text.num_layers = 4
    cfg, model = _model(cfg=cfg, stream=dict(size=224), max_len=1024)
    streams = [_stream_kw(cfg, 224, 3, t, q, window=128) for t, q in (("hello world", "Commentate on this match"), ("the game begins", "What happens now"),
                                                                      ("one two three", "Describe the scene"), ("", "Commentate on this match"))]
    solo, grouped = _solo_and_group(cfg, model, streams, 4)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def test_refused_configurations():
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model = _model("qwen2", True)
    group = StreamGroup(model._svlm_engine, 2)
    req = dict(ids=[1, 2, 3], cache=None, video_grid_thw=[], max_new_tokens=4)
    for extra in (dict(do_sample=True), dict(do_sample=True, top_k=5), dict(force_tokens=[1]), dict(keep_logits=True)):
        with pytest.raises(ValueError, match="stream group"):
            group.generate([dict(req, **extra), None])
    with pytest.raises(ValueError):
        StreamGroup(model._svlm_engine, 5)
