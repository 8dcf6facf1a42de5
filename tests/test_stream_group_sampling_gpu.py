"""Per-lane temperature / top-k / top-p sampling in stream groups.

Kernel layer: svlm_decb_lm_head_sample[_fp8] + svlm_decb_sample_finish against the single-row entries (svlm_dec_lm_head[_sample][_fp8] +
svlm_argmax_finish / svlm_penalty_sample) run once per lane on copies of that lane's buffers.  The bar is BITWISE equality of the token,
`state`, `seen` and the fp32 logits row: the batched kernels call the single-row bodies, so there is no tolerance.

End to end: per lane a sampling group must produce exactly what the same stream produces ALONE on a FRESH model built from the same
weights with the same generator seed (a call's Philox seed mixes in how many sampled calls the engine has made, so neither the solo
model nor a lane may have drawn before, and streams do not outnumber lanes).  The weights are iid N(0, 0.02): their next-token
distribution is close to uniform over 151680 ids, so a draw at T = 0.9 is the argmax with probability ~1e-5 per token and a sampled
stream cannot pass by coinciding with the greedy one -- which the test also asserts on the solo runs."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 128
# (temperature, top_k, top_p) per mode; top_k = 1 is the argmax
GREEDY, GUMBEL, FILTERED, NUCLEUS = (1.0, 1, 1.0), (0.9, 0, 1.0), (0.9, 50, 0.9), (0.9, 0, 0.9)
MODES = [GUMBEL, FILTERED, NUCLEUS, GREEDY]
STEPS = 3


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def same(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ bitwise"


class Lane:
    """What the head and the token choice touch of a lane, a sampling setting and a seed of its own."""

    def __init__(self, b, V, setting, limit=10, penalty=1.05, seen=True):
        g = torch.Generator().manual_seed(500 + 31 * b)
        self.pool = torch.zeros((1, 2, 1, 16, D), dtype=BF16).cuda()          # (the head never reads it; the record wants one)
        self.slot_of = torch.arange(16, dtype=torch.int32).cuda()
        self.state = torch.tensor([7 + 9 * b, 1 + b], dtype=torch.int32).cuda()
        self.tok_buf = torch.randint(0, V, (12,), generator=g).to(torch.int32).cuda()
        self.seen = (torch.rand(V, generator=g) < 0.3).to(torch.uint8).cuda() if seen else None
        self.rng = torch.tensor([1234567 + 1000003 * b, 89 + b], dtype=torch.int32).cuda()
        self.limit, self.penalty, self.n_suppress, self.setting = limit, penalty, 0, setting

    def records(self, ops):
        t, k, p = self.setting
        return (ops.lane_record(self.pool, None, self.slot_of, self.state, self.tok_buf, self.seen, self.limit, self.penalty, self.n_suppress),
                ops.lane_sample_record(self.rng, t, k, p))

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("state", "tok_buf", "seen") if getattr(self, k) is not None}


def tables(ops, lanes):
    recs = [ln.records(ops) for ln in lanes]
    return torch.from_numpy(np.stack([r[0] for r in recs])).cuda(), torch.from_numpy(np.stack([r[1] for r in recs])).cuda()


def single_row_choice(ops, ln, snap, logits, sup, ws):
    """The single stream's token choice on the copies in `snap`, from the logits row (top-k / top-p) or the candidates in `ws`."""
    t, k, p = ln.setting
    if ops.sample_mode(k, p) in (ops.SAMPLE_FILTERED, ops.SAMPLE_NUCLEUS):
        ops.penalty_sample(logits, snap.get("seen"), ln.penalty, sup, t, k, p, ln.rng, snap["tok_buf"], snap["state"], 1, ws)
    else:
        ops.argmax_finish(ws, logits.numel(), snap.get("seen"), snap["tok_buf"], snap["state"], 1)


_WEIGHTS = {}


def head_weights(fp8, V, K):
    """The lm_head of a case, made once on the GPU: bf16 rows, or e4m3 codes + power-of-two row scales over two decades of magnitude."""
    key = (fp8, V, K)
    if key not in _WEIGHTS:
        g = torch.Generator(device="cuda").manual_seed(7 + V)
        w = torch.randn((V, K), generator=g, device="cuda") / np.sqrt(K)
        if fp8:
            from streaming_vlm_amd.weights import quantize_rows_fp8_pow2
            w = w * 10.0 ** (torch.rand((V, 1), generator=g, device="cuda") * 2 - 1)
            q, s = quantize_rows_fp8_pow2(w.to(BF16))
            assert len(torch.unique(s)) >= 4, "the rows must not share one scale"
            _WEIGHTS[key] = (q.cuda(), s.cuda())
        else:
            _WEIGHTS[key] = (w.to(BF16),)
        _WEIGHTS[key + ("ln",)] = (1.0 + 0.1 * torch.randn(K, generator=g, device="cuda")).to(BF16)
    return _WEIGHTS[key], _WEIGHTS[key + ("ln",)]


# (V, K, B, parked lane): (1003, 256) takes the scalar tail of the row scan (V no multiple of 4 or 8), (4096, 512) its 16-B path, the
# last the real vocabulary at the 2B width; lane b of a batch of B runs MODES[(b + B) % 4], so every mode is met live at every shape
CASES = [(V, K, B, parked) for V, K in ((1003, 256), (4096, 512)) for B, parked in ((1, None), (2, 1), (3, 0), (4, 2), (4, None))]
CASES.append((151936, 1536, 4, 1))


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("V,K,B,parked", CASES)
def test_batched_sampling_is_bitwise_the_single_row_sampling_per_lane(ops, V, K, B, parked, fp8):
    W, ln_w = head_weights(fp8, V, K)
    lanes = [Lane(b, V, MODES[(b + B) % 4], limit=0 if b == parked else 10) for b in range(B)]
    live = [b for b in range(B) if b != parked]
    lanes[live[0]].n_suppress = 2                          # two suppressed ids on one lane, none on the others
    single_head = ops.dec_lm_head_fp8 if fp8 else ops.dec_lm_head
    batched_head = ops.decb_lm_head_sample_fp8 if fp8 else ops.decb_lm_head_sample
    suppress = torch.zeros(8, dtype=torch.int32).cuda()
    tab, smp = tables(ops, lanes)
    for b, ln in enumerate(lanes):                         # the record holds the host's fp32 quotient and the kernel the setting takes
        t, k, p = ln.setting
        assert smp[b, 1:2].cpu().numpy().view(np.float32)[0] == np.float32(1.0) / np.float32(t)
        assert int(smp[b, 2:3].cpu().numpy().view(np.int32)[1]) == ops.sample_mode(k, p)
    want = [ln.snapshot() for ln in lanes]
    frozen = lanes[parked].snapshot() if parked is not None else None
    logits = torch.full((B, V), -7.0, dtype=torch.float32).cuda()
    ws = ops.decb_sampling_ws(V, B, "cuda")
    for step in range(STEPS):
        g = torch.Generator().manual_seed(40 + 7 * B + step)
        x = (torch.randn((B, K), generator=g) * 2.0).to(BF16).cuda()
        if step == 0:        # the suppressed ids are that lane's two largest scores, so suppression decides what it may choose
            l0 = torch.zeros(V, dtype=torch.float32).cuda()
            single_head(x[live[0]], ln_w, 1e-6, *W, l0, None, 1.0, None, ops.sampling_ws(V, "cuda"))
            suppress[:2] = torch.topk(l0, 2).indices.to(torch.int32)
        # ---- yardstick: the single-row entries, lane by lane, on the copies
        rows = {}
        for b in live:
            ln, snap = lanes[b], want[b]
            t, k, p = ln.setting
            sup = suppress[:2] if ln.n_suppress else None
            row, sws = torch.zeros(V, dtype=torch.float32).cuda(), ops.sampling_ws(V, "cuda")
            kw = dict(temperature=t, rng=ln.rng, state=snap["state"]) if ops.sample_mode(k, p) == ops.SAMPLE_GUMBEL else {}
            single_head(x[b], ln_w, 1e-6, *W, row, snap["seen"], ln.penalty, sup, sws, **kw)
            single_row_choice(ops, ln, snap, row, sup, sws)
            rows[b] = row
        # ---- batched: one head launch and one finish launch for all lanes
        batched_head(tab, smp, B, x, ln_w, 1e-6, *W, logits, suppress, ws)
        ops.decb_sample_finish(tab, smp, B, logits, suppress, ws, V, 1)
        torch.cuda.synchronize()
        for b in live:
            same(f"step {step} logits[{b}]", logits[b], rows[b])
            for k, v in lanes[b].snapshot().items():
                same(f"step {step} lane {b} {k}", v, want[b][k])
            assert int(lanes[b].state[1]) == 2 + b + step, "the counter of the draws moves with every step"
    if parked is not None:
        for k, v in lanes[parked].snapshot().items():
            same(f"parked lane {k}", v, frozen[k])
        assert bool((logits[parked] == -7.0).all()), "the parked lane's logits row was written"


def test_filtered_lanes_take_the_multi_level_radix_descent_like_the_single_row_kernel(ops):
    """20000 scores per lane that all fall into ONE 11-bit radix bin (same exponent, same two leading mantissa bits), k = 50: the
    candidate range is narrowed by the second and third level of the descent (tests/test_kernels_gpu.py holds the single-row kernel to
    the oracle's distribution on this input; here the batched finish must repeat its draws bit for bit)."""
    V, B = 20000, 3
    lanes = [Lane(b, V, (0.9, 50, 0.9 if b == 2 else 1.0), penalty=1.0, seen=False) for b in range(B)]
    g = torch.Generator().manual_seed(77)
    logits = (8.0 + torch.rand((B, V), generator=g) * 0.99).cuda()
    tab, smp = tables(ops, lanes)
    suppress = torch.zeros(8, dtype=torch.int32).cuda()
    ws = ops.decb_sampling_ws(V, B, "cuda")
    want = [ln.snapshot() for ln in lanes]
    for step in range(STEPS):
        for b, ln in enumerate(lanes):
            single_row_choice(ops, ln, want[b], logits[b], None, ops.sampling_ws(V, "cuda"))
        ops.decb_sample_finish(tab, smp, B, logits, suppress, ws, V, 1)
        torch.cuda.synchronize()
        for b, ln in enumerate(lanes):
            for k, v in ln.snapshot().items():
                same(f"step {step} lane {b} {k}", v, want[b][k])
    drawn = [lanes[b].tok_buf[2 + b:2 + b + STEPS].tolist() for b in range(B)]
    top = [set(torch.topk(logits[b], 50).indices.tolist()) for b in range(B)]
    assert all(t in top[b] for b in range(B) for t in drawn[b]), "a draw fell outside the lane's 50 largest scores"


def test_bad_sampling_arguments_are_refused(ops):
    from streaming_vlm_amd import _lib
    V, K, B = 1003, 256, 2
    W, ln_w = head_weights(False, V, K)
    lanes = [Lane(b, V, MODES[b]) for b in range(B)]
    tab, smp = tables(ops, lanes)
    x = torch.zeros((B, K), dtype=BF16).cuda()
    logits, ws, suppress = torch.zeros((B, V)).cuda(), ops.decb_sampling_ws(V, B, "cuda"), torch.zeros(8, dtype=torch.int32).cuda()
    with pytest.raises(_lib.SvlmError):
        ops.decb_lm_head_sample(tab, smp[:, :2].contiguous(), B, x, ln_w, 1e-6, *W, logits, suppress, ws)      # malformed sample table
    with pytest.raises(_lib.SvlmError):
        ops.decb_sample_finish(tab, smp[:1], B, logits, suppress, ws, V, 1)                                      # fewer records than lanes
    with pytest.raises(_lib.SvlmError):
        ops.decb_sample_finish(tab, smp, B, logits[:1], suppress, ws, V, 1)                                      # fewer rows than lanes
    with pytest.raises(_lib.SvlmError):
        # 16-B loads of the row scan: a vocabulary that is a multiple of 4 in rows that are not 16-B apart
        ops.decb_sample_finish(tab, smp, B, torch.zeros((B, 1001)).cuda(), suppress, ops.decb_sampling_ws(1000, B, "cuda"), 1000, 1)


# ================================================================ end to end
def _weights(cfg, decisive=None):
    from streaming_vlm_amd.weights import random_state_dict
    sd = random_state_dict(cfg, 3) if decisive is None else decisive
    return {k: v.cuda() for k, v in sd.items()}


def _fresh(cfg, sd, use_graph=True, max_new=8, **kw):
    import streaming_vlm_amd as S
    return S.StreamingQwen2VL(cfg, sd, "cuda", max_len=768, max_new_tokens=max_new, use_graph=use_graph, **kw)


def _stream_kw(cfg, size, n_chunks, previous_text, query, sampling, seed, max_new=8, suppress_eos=True, window=64):
    size_s = f"{size[1]}x{size[0]}" if isinstance(size, (tuple, list)) else f"{size}x{size}"
    kw = dict(video_path=f"synthetic://{size_s}@1fps", model_base="Qwen2_5" if cfg.family == "qwen2_5" else "Qwen2", duration=n_chunks,
              previous_text=previous_text, query=query, kv_policy="sink_window", sink=4, window=window, max_new_tokens=max_new,
              suppress_eos=suppress_eos, quiet=True, do_sample=False)
    if sampling is not None:
        t, k, p = sampling
        kw.update(do_sample=True, temperature=t, top_k=k, top_p=p, seed=seed)
    return kw


def _run(fn, kw):
    """One stream with its logs; `seed` becomes a generator of the run's own (a generator object must not be shared between runs)."""
    kw = dict(kw)
    seed = kw.pop("seed", None)
    if seed is not None:
        kw["generator"] = torch.Generator().manual_seed(seed)
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


def _solo(cfg, sd, stream, **model_kw):
    """The stream alone on a FRESH model (its engine has made no sampled call yet)."""
    import streaming_vlm_amd as S
    model = _fresh(cfg, sd, **model_kw)
    return _run(lambda kw: S.streaming_inference(model=model, processor=S.SyntheticProcessor(), **kw), stream)


def _group(cfg, sd, streams, sampling=True, **model_kw):
    """The streams on as many lanes of a fresh model's group."""
    import streaming_vlm_amd as S
    model = _fresh(cfg, sd, **model_kw)
    logs = [dict(trace=[], token_counts=[], ids_log=[]) for _ in streams]
    kws = []
    for s, lg in zip(streams, logs):
        s = dict(s, **lg)
        seed = s.pop("seed", None)
        if seed is not None:
            s["generator"] = torch.Generator().manual_seed(seed)
        kws.append(s)
    res = S.streaming_inference_group(model, S.SyntheticProcessor(), kws, n_lanes=len(streams), sampling=sampling)
    return list(zip(res, logs))


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_three_sampled_streams_in_lock_step_equal_their_solo_runs(family, use_graph):
    """Plain temperature, top-k with top-p, and top-p alone on three lanes, a seed per stream; the second stream ends four chunks before
    the others; the window makes every stream evict at least twice."""
    from streaming_vlm_amd import config as C
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = _weights(cfg)
    streams = [_stream_kw(cfg, 56, 9, "hello world", "Commentate on this match", GUMBEL, 11),
               _stream_kw(cfg, (112, 84), 5, "the game begins", "What happens now", FILTERED, 22, window=96),
               _stream_kw(cfg, 84, 9, "", "Describe the scene", (1.3, 0, 0.9), 33)]
    solo = [_solo(cfg, sd, s, use_graph=use_graph) for s in streams]
    grouped = _group(cfg, sd, streams, use_graph=use_graph)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        assert sum(1 for t in w[1]["trace"] if t) >= 2, f"stream {i} must evict at least twice for this test to mean anything: {w[1]['trace']}"
        _same_stream(i, g, w)
    # not a greedy run in disguise: the sampled stream differs from the greedy run of the same input, and from another seed's draws
    greedy = _solo(cfg, sd, dict(streams[0], do_sample=False, seed=None), use_graph=use_graph)
    assert [r["response"] for r in greedy[0]] != [r["response"] for r in solo[0][0]], "T = 0.9 reproduced the argmax on these weights"
    other = _solo(cfg, sd, dict(streams[0], seed=12), use_graph=use_graph)
    assert [r["response"] for r in other[0]] != [r["response"] for r in solo[0][0]], "the generator seed does not reach the draws"


def test_two_lanes_on_fp8_weights_greedy_beside_top_k():
    from streaming_vlm_amd import config as C
    cfg = C.tiny()
    sd = _weights(cfg)
    streams = [_stream_kw(cfg, 56, 5, "hello world", "Commentate on this match", None, None),
               _stream_kw(cfg, 84, 5, "the game begins", "What happens now", (0.9, 50, 1.0), 5)]
    solo = [_solo(cfg, sd, s, llm_fp8=True) for s in streams]
    grouped = _group(cfg, sd, streams, llm_fp8=True)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def test_a_sampled_lane_that_meets_eos_mid_chunk_is_parked_while_the_others_go_on():
    """Copy-head weights whose copy walks over the prompt's closing <|im_end|> (tests/test_stream_group_gpu.py): the lane that meets it
    draws through the top-k kernel at T = 0.05 (cold enough that the draw follows the copy head to the marker; the path is the sampled
    one all the same), its neighbours through the Gumbel head and the argmax; where the solo run stops is found first."""
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.config import IM_END
    from streaming_vlm_amd.weights import decisive_state_dict
    cfg = C.tiny()
    for offset in (10, 11, 9, 12, 8, 13, 14):
        sd = decisive_state_dict(cfg, 0, "cpu", offset=offset)
        emb = next(v for k, v in sd.items() if k.endswith("embed_tokens.weight"))
        emb[IM_END] = (torch.randn(emb.shape[1], generator=torch.Generator().manual_seed(5)) * 0.02).to(emb.dtype)
        sd = _weights(cfg, sd)
        streams = [_stream_kw(cfg, 56, 6, "hello world", "Commentate on this match", (0.05, 50, 1.0), 7, max_new=16, suppress_eos=False),
                   _stream_kw(cfg, 56, 6, "the game begins", "What happens now", GUMBEL, 8, max_new=5),
                   _stream_kw(cfg, 84, 6, "a b c", "Describe the scene", None, None, max_new=12)]
        first = _solo(cfg, sd, streams[0], max_new=16)
        print(f"copy offset {offset}: solo token counts of the EOS stream: {first[1]['token_counts']}")
        if any(4 < c < 16 for c in first[1]["token_counts"]):
            break
    else:
        raise AssertionError("no copy offset makes the sampled solo stream stop mid-chunk")
    solo = [first] + [_solo(cfg, sd, s, max_new=16) for s in streams[1:]]
    grouped = _group(cfg, sd, streams, max_new=16)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        _same_stream(i, g, w)


def test_a_sampling_group_given_greedy_requests_is_the_greedy_group():
    from streaming_vlm_amd import config as C
    cfg = C.tiny()
    sd = _weights(cfg)
    streams = [_stream_kw(cfg, 56, 4, "hello world", "Commentate on this match", None, None),
               _stream_kw(cfg, 84, 4, "the game begins", "What happens now", None, None),
               dict(_stream_kw(cfg, 56, 4, "a b c", "Describe the scene", None, None), do_sample=True, top_k=1)]
    plain = _group(cfg, sd, streams, sampling=False)
    sampling = _group(cfg, sd, streams, sampling=True)
    for i, (g, w) in enumerate(zip(sampling, plain)):
        _same_stream(i, g, w)
