"""Stream groups with batched_attn=True (one lane-batched decode-attention launch pair per layer, svlm_decb_attn) end to end, tiny config.

Per lane svlm_decb_attn is bitwise the single-lane attention (tests/test_decode_attn_batch_gpu.py) and nothing else in the step changes,
so a group with the flag must reproduce THE SAME GROUP WITHOUT IT exactly: responses, token counts, logical id order, cache lengths,
eviction traces and, per stream and chunk, the lane's logits after the chunk's last decode step (bitwise; filed by stream, because which
lane a stream runs in and which row of the group's buffers a lane has are not fixed).  Covered: a narrow bf16 group, wide groups of 8
and 16, an llm_fp4 group, a sampling group (same seeds, fresh models), a lane that stops at an EOS mid-chunk, and graph replay over
many chunks (the attention table is rewritten between replays)."""
import pytest
import torch

import helpers as H
from test_stream_group_wide_gpu import PROMPTS, _eight_streams, _model, _same_stream, _stream_kw

pytestmark = pytest.mark.gpu


def _group_run(model, streams, n_lanes, use_graph=True, seeds=None, **group_kw):
    """The streams on a fresh group of `model` -> ([(responses, logs)], per stream the logits row of its lane after the last step of every
    chunk).  Which lane a stream runs in is decided by the lane threads' race for the queue and which row of the group's buffers a lane
    has by who else is in the batch, so the rows are filed by STREAM: every batch's rows are copied after it ran, under the lane they
    belong to, and each stream notes the lane whose thread runs it."""
    import threading
    import streaming_vlm_amd as S
    from streaming_vlm_amd.stream_group import StreamGroup
    group = StreamGroup(model._svlm_engine, n_lanes, **group_kw)
    assert group.batched_attn == bool(group_kw.get("batched_attn")) and (group.attn_table is not None) == group.batched_attn
    group.use_graph = use_graph
    per_lane = [[] for _ in range(n_lanes)]
    generate = group.generate

    def generate_and_keep_logits(requests, **kw):
        out = generate(requests, **kw)
        torch.cuda.synchronize()
        live = [i for i, r in enumerate(requests) if r is not None]
        assert not any(isinstance(out[i], BaseException) for i in live), [out[i] for i in live]
        for j, i in enumerate(live):                 # row j of the group's buffers was lane i's in this batch
            per_lane[i].append(group.logits[j].clone())
        return out

    group.generate = generate_and_keep_logits         # (the rendezvous looks `generate` up on the group at every batch)
    lane_of = {}
    logs = [dict(trace=[], token_counts=[], ids_log=[]) for _ in streams]
    kws = [dict(s, **lg) for s, lg in zip(streams, logs)]
    for si, kw in enumerate(kws):
        kw["chunk_callback"] = lambda _chunk, si=si: lane_of.setdefault(si, int(threading.current_thread().name.rsplit("-", 1)[1]))
    for kw, seed in zip(kws, seeds or []):
        if seed is not None:
            kw["generator"] = torch.Generator().manual_seed(seed)
    assert len(streams) <= n_lanes                    # one stream per lane: a lane's rows are one stream's
    res = S.streaming_inference_group(model, S.SyntheticProcessor(), kws, group=group)
    torch.cuda.synchronize()
    assert sorted(lane_of) == list(range(len(streams))) and len(set(lane_of.values())) == len(streams), lane_of
    return list(zip(res, logs)), [per_lane[lane_of[si]] for si in range(len(streams))]


def _same_logits(flag, plain):
    """Per stream and chunk, the lane's logits row after the chunk's last decode step: bitwise."""
    assert len(flag) == len(plain)
    for si, (f, p) in enumerate(zip(flag, plain)):
        assert len(f) == len(p) and len(p) > 0, f"stream {si}: {len(f)} / {len(p)} chunks"
        for ci, (a, b) in enumerate(zip(f, p)):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"stream {si} chunk {ci}: the logits of the last step differ bitwise"


def _with_and_without(model, streams, n_lanes, use_graph=True, min_chunks=1, **group_kw):
    plain, logits_p = _group_run(model, streams, n_lanes, use_graph, **group_kw)
    flag, logits_f = _group_run(model, streams, n_lanes, use_graph, batched_attn=True, **group_kw)
    assert max(len(p[1]["token_counts"]) for p in plain) >= min_chunks
    for i, (g, w) in enumerate(zip(flag, plain)):
        assert sum(w[1]["token_counts"]) > len(w[1]["token_counts"]), f"stream {i} took no decode step"
        assert len(logits_p[i]) == len(w[1]["token_counts"]), f"stream {i}: a logits row per chunk"
        _same_stream(i, g, w)
    _same_logits(logits_f, logits_p)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_a_narrow_group_of_three(use_graph):
    """Different prompts, frame sizes, chunk counts and windows; with the graph the step is replayed over 9 chunks of which every one
    rewrites the attention table (new rope table rows, evictions, another attn_len as the caches grow)."""
    cfg, model, _ = _model()
    streams = _eight_streams(cfg)[:3]
    _with_and_without(model, streams, 3, use_graph, min_chunks=9)


def test_a_wide_group_of_eight():
    cfg, model, _ = _model()
    _with_and_without(model, _eight_streams(cfg), 8, wide=True, min_chunks=9)


def test_a_wide_group_of_sixteen_on_random_weights():
    """Random weights: no greedy margin absorbs anything, a single differing bit of an attention row would move the tokens."""
    cfg, model, _ = _model("random")
    sizes = [56, 84, (112, 84), 56]
    streams = [_stream_kw(cfg, sizes[i % 4], 3, PROMPTS[i % 8][0] + (" x" * (i // 8)), PROMPTS[(i + 3) % 8][1], max_new=8 - i % 3) for i in range(16)]
    _with_and_without(model, streams, 16, wide=True, min_chunks=3)


def test_an_fp4_group_of_two():
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    cfg = C.tiny()
    sd = H.decisive_weights(cfg, size=(112, 84), max_new=8)
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=8, llm_fp4=True)
    streams = [_stream_kw(cfg, 56, 5, "hello world", "Commentate on this match"), _stream_kw(cfg, (112, 84), 4, "the game begins", "What happens now", window=96)]
    _with_and_without(model, streams, 2, min_chunks=5)


def test_a_sampling_group_of_two_with_the_same_seeds():
    """A call's Philox seed mixes in how many sampled calls the engine has made: each run gets a fresh model."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    cfg = C.tiny()
    sd = {k: v.cuda() for k, v in random_state_dict(cfg, 3).items()}
    streams = [dict(_stream_kw(cfg, 56, 5, "hello world", "Commentate on this match"), do_sample=True, temperature=0.9, top_k=0, top_p=1.0),
               dict(_stream_kw(cfg, 84, 5, "the game begins", "What happens now"), do_sample=True, temperature=0.8, top_k=40, top_p=0.95)]
    runs = []
    for flag in (False, True):
        model = S.StreamingQwen2VL(cfg, sd, "cuda", max_len=768, max_new_tokens=8)
        runs.append(_group_run(model, streams, 2, seeds=[11, 22], sampling=True, **({"batched_attn": True} if flag else {})))
    (plain, logits_p), (flag, logits_f) = runs
    for i, (g, w) in enumerate(zip(flag, plain)):
        _same_stream(i, g, w)
    _same_logits(logits_f, logits_p)


def test_a_lane_that_meets_eos_mid_chunk():
    """The construction of tests/test_stream_group_wide_gpu.py: the copy head walks over the prompt's closing <|im_end|> a few steps into
    a chunk, the lane is parked (limit 0: not live) and the batched attention must skip it while the others go on."""
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.config import IM_END
    from streaming_vlm_amd.weights import decisive_state_dict
    cfg = C.tiny()
    streams = [_stream_kw(cfg, 56, 6, "hello world", "Commentate on this match", max_new=16, suppress_eos=False),
               _stream_kw(cfg, 56, 6, "the game begins", "What happens now", max_new=5),
               _stream_kw(cfg, 84, 6, "a b c", "Describe the scene", max_new=12)]
    for offset in (10, 11, 9, 12, 8, 13, 14):
        sd = decisive_state_dict(cfg, 0, "cpu", offset=offset)
        emb = next(v for k, v in sd.items() if k.endswith("embed_tokens.weight"))
        emb[IM_END] = (torch.randn(emb.shape[1], generator=torch.Generator().manual_seed(5)) * 0.02).to(emb.dtype)
        model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", max_len=768, max_new_tokens=16)
        plain, logits_p = _group_run(model, streams, 3)
        counts = plain[0][1]["token_counts"]
        if any(4 < c < 16 for c in counts):
            break
    else:
        raise AssertionError("no copy offset makes the first stream stop mid-chunk")
    flag, logits_f = _group_run(model, streams, 3, batched_attn=True)
    for i, (g, w) in enumerate(zip(flag, plain)):
        _same_stream(i, g, w)
    _same_logits(logits_f, logits_p)


def test_the_flag_on_a_real_engine():
    from streaming_vlm_amd.stream_group import StreamGroup
    cfg, model, _ = _model()
    group = StreamGroup(model._svlm_engine, 2, batched_attn=True)
    assert tuple(group.attn_table.shape) == (2, model._svlm_engine.ops.ATTN_WORDS) and group._attn_table_host.is_pinned()
    assert StreamGroup(model._svlm_engine, 2).attn_table is None
