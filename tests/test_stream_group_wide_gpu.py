"""Wide stream groups (StreamGroup(wide=True): the decode step's weight kernels on the MFMA, up to 16 lanes) end to end, tiny config.

Two yardsticks.  On the decisive weights (greedy margins tens of times the bf16 noise) every stream of a wide group equals the stream run
ALONE on a plain engine exactly: responses, eviction traces, token counts, logical ids and cache lengths -- the wide kernels sum in
another order than the single-row ones, which the margins absorb.  On random, non-decisive weights that comparison would not hold, but
LANE INDEPENDENCE does, without margins: a stream in a wide group of 8 equals the same stream in a wide group of ONE exactly."""
import pytest
import torch

import helpers as H

pytestmark = pytest.mark.gpu

PROMPTS = [("hello world", "Commentate on this match"), ("the game begins", "What happens now"), ("", "Describe the scene"),
           ("one two three", "Describe the scene"), ("a b c", "What happens now"), ("red green blue", "Commentate on this match"),
           ("", "What happens now"), ("north south", "Describe the scene")]
_MODEL = {}


def _model(kind="decisive"):
    """One tiny model per weight kind for the whole module (the solo runs are shared too)."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    if kind not in _MODEL:
        cfg = C.tiny()
        sd = H.decisive_weights(cfg, size=(112, 84), max_new=8) if kind == "decisive" else random_state_dict(cfg, seed=3)
        _MODEL[kind] = (cfg, S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8), {})
    return _MODEL[kind]


def _stream_kw(cfg, size, n_chunks, previous_text, query, max_new=8, suppress_eos=True, window=64, fps=1.0):
    size_s = f"{size[1]}x{size[0]}" if isinstance(size, (tuple, list)) else f"{size}x{size}"
    return dict(video_path=f"synthetic://{size_s}@{fps:g}fps", model_base="Qwen2", duration=n_chunks, previous_text=previous_text, query=query,
                kv_policy="sink_window", sink=4, window=window, do_sample=False, max_new_tokens=max_new, suppress_eos=suppress_eos, quiet=True)


def _run(fn, kw):
    logs = dict(trace=[], token_counts=[], ids_log=[])
    return fn(dict(kw, **logs)), logs


def _same_stream(i, got, want):
    (gr, gl), (wr, wl) = got, want
    assert [r["response"] for r in gr] == [r["response"] for r in wr], f"stream {i}: responses differ"
    assert gl["trace"] == wl["trace"], f"stream {i}: eviction traces differ"
    assert gl["token_counts"] == wl["token_counts"], f"stream {i}: n_new per chunk differs"
    assert len(gl["ids_log"]) == len(wl["ids_log"])
    for c, (a, b) in enumerate(zip(gl["ids_log"], wl["ids_log"])):
        assert a["ids"] == b["ids"] and a["new"] == b["new"], f"stream {i} chunk {c}: logical id order / new tokens differ"
        assert a["kv_len"] == b["kv_len"], f"stream {i} chunk {c}: cache length differs"


def _solo(model, memo, streams):
    """Each stream alone on the plain engine (memoised per stream: the graph and no-graph cases share them)."""
    import streaming_vlm_amd as S
    proc = S.SyntheticProcessor()
    out = []
    for s in streams:
        key = repr(sorted(s.items()))
        if key not in memo:
            memo[key] = _run(lambda kw: S.streaming_inference(model=model, processor=proc, **kw), s)
        out.append(memo[key])
    return out


def _wide(model, streams, n_lanes, use_graph=True):
    import streaming_vlm_amd as S
    from streaming_vlm_amd.stream_group import StreamGroup
    group = StreamGroup(model._svlm_engine, n_lanes, wide=True)
    assert group.wide and group.n_lanes == n_lanes
    group.use_graph = use_graph
    logs = [dict(trace=[], token_counts=[], ids_log=[]) for _ in streams]
    res = S.streaming_inference_group(model, S.SyntheticProcessor(), [dict(s, **lg) for s, lg in zip(streams, logs)], group=group)
    return list(zip(res, logs))


def _eight_streams(cfg):
    """Different prompts, frame sizes, chunk counts and max_new_tokens; streams 1 and 5 end early."""
    sizes = [56, (112, 84), 84, 56, 84, (112, 84), 56, 84]
    chunks = [9, 5, 9, 8, 9, 6, 9, 8]
    windows = [64, 96, 64, 64, 64, 96, 64, 64]
    max_new = [8, 8, 6, 7, 8, 5, 8, 7]
    return [_stream_kw(cfg, sizes[i], chunks[i], *PROMPTS[i], max_new=max_new[i], window=windows[i]) for i in range(8)]


@pytest.mark.parametrize("use_graph", [True, False])
def test_eight_streams_on_eight_wide_lanes_equal_their_solo_runs(use_graph):
    cfg, model, memo = _model()
    streams = _eight_streams(cfg)
    solo = _solo(model, memo, streams)
    grouped = _wide(model, streams, 8, use_graph)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        assert sum(1 for t in w[1]["trace"] if t) >= 2, f"stream {i} must evict at least twice for this test to mean anything: {w[1]['trace']}"
        _same_stream(i, g, w)


def test_sixteen_wide_lanes_three_short_chunks_equal_their_solo_runs():
    cfg, model, memo = _model()
    sizes = [56, 84, (112, 84), 56]
    streams = [_stream_kw(cfg, sizes[i % 4], 3, PROMPTS[i % 8][0] + (" x" * (i // 8)), PROMPTS[(i + 3) % 8][1], max_new=8 - i % 3) for i in range(16)]
    solo = _solo(model, memo, streams)
    grouped = _wide(model, streams, 16)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def test_random_weights_eight_wide_lanes_equal_wide_groups_of_one():
    """Lane independence end to end, on weights whose greedy margins are NOT wide: no comparison with the single-row kernels could be
    exact here, the comparison of a wide lane with itself alone is."""
    cfg, model, _ = _model("random")
    streams = [dict(s, duration=4) for s in _eight_streams(cfg)]
    grouped = _wide(model, streams, 8)
    for i, s in enumerate(streams):
        alone = _wide(model, [s], 1)[0]
        _same_stream(i, grouped[i], alone)


def test_a_wide_lane_that_meets_eos_mid_chunk_is_parked_and_the_others_are_unaffected():
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.config import IM_END
    from streaming_vlm_amd.weights import decisive_state_dict
    cfg = C.tiny()
    # as tests/test_stream_group_gpu.py: the copy head walks over the prompt's closing <|im_end|> a few steps into a chunk; the first
    # copy offset whose SOLO run stops mid-chunk (past the first EOS look at step 4) is the case
    for offset in (10, 11, 9, 12, 8, 13, 14):
        sd = decisive_state_dict(cfg, 0, "cpu", offset=offset)
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
    solo = _solo(model, {}, streams)
    assert solo[0][1]["token_counts"] == counts
    grouped = _wide(model, streams, 3)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def test_wide_refusals_on_a_real_engine():
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model, _ = _model()
    eng = model._svlm_engine
    with pytest.raises(ValueError, match="wide=True"):
        StreamGroup(eng, 17, wide=True)
    with pytest.raises(ValueError, match="wide=True"):
        StreamGroup(eng, 2, sampling=True, wide=True)
    with pytest.raises(ValueError):
        StreamGroup(eng, 5)
    group = StreamGroup(eng, 2, wide=True)
    with pytest.raises(ValueError, match="stream group"):
        group.generate([dict(ids=[1, 2, 3], cache=None, video_grid_thw=[], max_new_tokens=4, do_sample=True, top_k=5), None])
