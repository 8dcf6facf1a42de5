"""Stream groups: B independent streams (B = 1..4, "lanes"; 1..16 in a wide group, below) on one GPU and ONE weight set, whose decode steps run in lock-step through
the lane-batched kernels of csrc/decode_batch.hip -- each weight byte is read once and each launch boundary paid once for B tokens.
An `llm_fp8=True` engine takes the same steps through the e4m3 twins of csrc/decode_batch_fp8.hip: half the weight bytes, read once
for B tokens, and each weight converted to fp32 once for all B lanes.  Its prefill stays per stream and dequantises layer by layer
into ONE bf16 scratch layer that all lanes share (a group pays that dequantisation once per lane and chunk).
An `llm_fp4=True` engine takes them through the MXFP4 twins of csrc/decode_batch_fp4.hip (e2m1 codes + e8m0 block scales, a quarter of
the bf16 bytes, each half block converted once for all B lanes) and the e4m3 head; with `prefill_fp4=True` every lane's prefill reads
the codes directly, otherwise (or for a pass above `PREFILL_FP4_MAX_ROWS`) the lanes share the one scratch layer as fp8 lanes do.

A lane is an `SvlmEngine` that shares the group engine's weights (`SvlmEngine(share=...)`; lane 0 IS the group engine) and owns
everything a stream owns: KV pool, positions, rope table, sampling state, eviction history.  `StreamGroup.generate` runs
`generate_begin` lane after lane (the prefill stays per stream), then the lock-step batched decode steps, then `generate_finish` per
lane; per lane the tokens, cache length and logical order are EXACTLY those of the stream run alone (the batched kernels are bitwise
the single-row ones per lane, and the decode attention is the unchanged single-stream kernel, launched once per lane).

Batched attention.  `StreamGroup(..., batched_attn=True)` replaces those per-lane launches -- `2 * B * n_layers` per step -- by one
`decb_attn` per layer (csrc/decode_attn.hip, svlm_decb_attn: the same kernels with the lane as a third grid dimension, one split and one
combine launch for all lanes).  The group keeps a table of `svlm_lane_attn` records parallel to the lane table (rope table, lin_state,
workspace, and the `attn_len` / `decode_chunk` the lane's `generate_begin` picked for this call), rewritten at the start of every
`generate()`.  Per lane the attention is bitwise the single-stream kernel's, so the flag changes no token; it combines with `wide`,
`sampling` and fp8 / fp4 engines.  An ops backend without `decb_attn` is refused with a ValueError that names `batched_attn=True`.

Token choice.  By default a group is greedy.  `StreamGroup(..., sampling=True)` batches the reference's default token choice as well:
every lane's request carries its own `do_sample / temperature / top_k / top_p / generator`, and one batch may mix greedy, plain
temperature, top-k (with or without top-p) and top-p alone.  `generate_begin` draws a lane's first token with the single-row kernels and
sets the lane's Philox seed (`lane.rng_dev`) as it does for a stream alone; the group then writes one `svlm_lane_sample` record per lane
(seed pointer, fp32 1/T, k, p and the kernel the setting takes) next to the lane record, and a step with any sampled lane ends in
`decb_lm_head_sample[_fp8]` + `decb_sample_finish` (one workgroup per lane, all lanes in one launch) instead of `decb_lm_head[_fp8]` +
`decb_argmax_finish`.  Per lane the draws are bitwise the single-row ones, so the tokens are those of the stream run alone on a fresh
engine with the same generator seed (a seed mixes in how many sampled calls the lane's engine has made).

Opt-in; nothing here is reached by the single-stream path.  Refused with a ValueError instead of silently falling back:
`decode_tail=True` engines, an `llm_fp8=True` engine whose ops backend lacks the batched fp8 entry points (with `sampling=True` also the
fp8 sampling head), an `llm_fp4=True` engine whose ops backend lacks the batched fp4 entry points or the batched fp8 head (with
`sampling=True` also the fp8 sampling head), `do_sample=True` with anything but `top_k == 1` unless the group was built with `sampling=True`, `force_tokens`,
`keep_logits`.

Wide groups.  `StreamGroup(..., wide=True)` takes the same steps through the `decw_*` entries of csrc/decode_wide.hip: the weight kernels
as skinny GEMMs on the matrix cores, whose cost is flat in the lane count, for 1..`MAX_LANES_WIDE` (16) lanes.  bf16 language-model
weights and greedy decoding only: an `llm_fp8=True` or `llm_fp4=True` engine, `sampling=True` and an ops backend without the `decw_*`
entry points are refused with a ValueError that names `wide=True`.  The launch sequence is the one above with `decw_` for `decb_`.  The
wide kernels keep the normalised rows and every rounding point of the single-row kernels but sum the dot products in another order, so a
lane is no longer bitwise the stream run alone; what holds instead is LANE INDEPENDENCE -- a lane's outputs do not depend on how many
lanes the batch has, on the lane's place in it or on what the other lanes hold -- so a stream in a wide group of 16 is exactly the
stream in a wide group of one.

The look-ahead ViT (`next_vision`) is DECLINED: a group runs strict-causal, every chunk's vision tower runs inside its own
`generate_begin`.
"""
from __future__ import annotations

import inspect
import math
import threading
import time
import weakref
from types import MethodType
from typing import Callable, List, Optional, Sequence

import numpy as np
import torch

from .engine import BF16, GenerateOutput, SvlmEngine

MAX_LANES = 4
# aggregate frames/s stops growing at 3 lanes on Qwen2-VL-2B (profiles/stream_group_2b.json: 4 lanes are 0.6 % below 3), so nothing picks
# more than 3 by itself; 4 remain available on request
DEFAULT_LANES = 3
# a wide group (wide=True): one lane per column of the 16-wide MFMA tile (csrc/decode_wide.hip, svlm_decw_max_lanes)
MAX_LANES_WIDE = 16
WIDE_GROUP_OPS = ("decw_embed", "decw_qkv", "decw_gemv", "decw_gate_up", "decw_lm_head", "decw_argmax_finish")
# ... and a group with batched_attn=True (csrc/decode_attn.hip, svlm_decb_attn)
ATTN_GROUP_OPS = ("decb_attn", "lane_attn_record")
# ops entry points a group on an llm_fp8 engine needs (csrc/decode_batch_fp8.hip)
FP8_GROUP_OPS = ("decb_qkv_fp8", "decb_gate_up_fp8", "decb_gemv_fp8", "decb_lm_head_fp8")
# ... and on an llm_fp4 engine (csrc/decode_batch_fp4.hip; the lm_head of an fp4 engine is e4m3)
FP4_GROUP_OPS = ("decb_qkv_fp4", "decb_gate_up_fp4", "decb_gemv_fp4", "decb_lm_head_fp8")


def check_request(req: dict, sampling: bool = False) -> dict:
    """Validate one lane's request (the keyword arguments of `SvlmEngine.generate`); returns it without the declined `next_vision`.
    `sampling`: the group batches sampled lanes (`StreamGroup(sampling=True)`), so every setting `generate_begin` accepts passes."""
    req = dict(req)
    req.pop("next_vision", None)
    if req.get("force_tokens") is not None:
        raise ValueError("stream group: force_tokens (teacher forcing) is a single-stream parity aid and is not supported")
    if req.get("keep_logits"):
        raise ValueError("stream group: keep_logits is not supported (the per-step logits of a lane stay on the device)")
    if not sampling and req.get("do_sample") and req.get("top_k") != 1:
        raise ValueError("stream group: only greedy decoding is batched unless the group was built with sampling=True; do_sample=True needs top_k=1 "
                         f"(got top_k={req.get('top_k')!r}, top_p={req.get('top_p')!r})")
    return req


class LaneRendezvous:
    """Host-side rendezvous of the lanes' threads.  A lane thread `attach`es, then calls `submit(i, request)` per chunk and blocks;
    the batch runs when EVERY attached lane has a request pending, on the thread whose arrival (or whose neighbour's `detach`)
    completed it -- all GPU work of a batch is issued from that one thread.  `run_batch(requests)` gets one request or None per
    lane and returns one result per lane; a result that is an exception is raised in that lane's `submit` only."""

    def __init__(self, n_lanes: int, run_batch: Callable[[List[Optional[dict]]], Sequence]):
        self.n_lanes = int(n_lanes)
        self._run = run_batch
        self._cv = threading.Condition()
        self._attached, self._pending, self._results = set(), {}, {}
        self._running = False
        self.batches = 0

    def attach(self, i: int) -> None:
        with self._cv:
            if not 0 <= i < self.n_lanes or i in self._attached:
                raise ValueError(f"lane {i} is out of range or already attached")
            self._attached.add(i)

    def detach(self, i: int) -> None:
        """The lane's stream has ended (or raised): the others carry on with a smaller batch."""
        with self._cv:
            self._attached.discard(i)
            self._pending.pop(i, None)
            self._cv.notify_all()

    def submit(self, i: int, request: dict, timeout: Optional[float] = None):
        deadline = None if timeout is None else time.monotonic() + timeout
        with self._cv:
            if i not in self._attached or i in self._pending:
                raise RuntimeError(f"lane {i} is not attached or already has a request pending")
            self._pending[i] = request
            while True:
                if i in self._results:
                    out = self._results.pop(i)
                    if isinstance(out, BaseException):
                        raise out
                    return out
                if not self._running and i in self._pending and self._attached <= self._pending.keys():
                    batch, self._pending = self._pending, {}
                    self._running = True
                    self._cv.release()
                    try:
                        try:
                            out = list(self._run([batch.get(k) for k in range(self.n_lanes)]))
                        except BaseException as e:       # the batch as a whole failed: every lane of it hears about it
                            out = [e] * self.n_lanes
                    finally:
                        self._cv.acquire()
                    for k in batch:
                        self._results[k] = out[k]
                    self._running = False
                    self.batches += 1
                    self._cv.notify_all()
                    continue
                left = None if deadline is None else deadline - time.monotonic()
                if left is not None and left <= 0:
                    self._pending.pop(i, None)
                    raise TimeoutError(f"lane {i}: no batch within {timeout} s")
                self._cv.wait(left)


class _LaneEngine:
    """What a lane model shows as `_svlm_engine`: the lane's engine, with `generate` handed to the group."""

    _SIG = inspect.signature(SvlmEngine.generate)

    def __init__(self, group: "StreamGroup", i: int):
        self._group, self._i, self._eng = group, i, group.lanes[i]

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def generate(self, *args, **kw) -> GenerateOutput:
        req = dict(self._SIG.bind(None, *args, **kw).arguments)
        req.pop("self")
        return self._group.submit(self._i, req)


class LaneModel:
    """The surface `streaming_inference` uses of a model (`.config`, `.device`, `._svlm_engine`, `.generate`, `.new_cache`) for one
    lane: `generate` hands its request to the group and waits for the batch."""

    def __init__(self, group: "StreamGroup", i: int):
        from .model import streaming_generate
        self.config = group.lanes[i].cfg
        self.device = group.lanes[i].device
        self._svlm_engine = _LaneEngine(group, i)
        self.generate = MethodType(streaming_generate, self)

    def new_cache(self):
        return self._svlm_engine.new_cache()


class StreamGroup:
    def __init__(self, engine: SvlmEngine, n_lanes: int = 2, sampling: bool = False, wide: bool = False, batched_attn: bool = False):
        max_lanes = MAX_LANES_WIDE if wide else MAX_LANES
        if not 1 <= int(n_lanes) <= max_lanes:
            raise ValueError(f"n_lanes={n_lanes} outside [1, {max_lanes}]" + (" (wide=True)" if wide else ""))
        if wide:
            if getattr(engine, "llm_fp8", False):
                raise ValueError("stream group: wide=True needs bf16 language-model weights; an llm_fp8=True engine is not supported")
            if getattr(engine, "llm_fp4", False):
                raise ValueError("stream group: wide=True needs bf16 language-model weights; an llm_fp4=True engine is not supported")
            if sampling:
                raise ValueError("stream group: wide=True is greedy only; sampling=True is not supported (there is no wide sampling head)")
            missing = [m for m in WIDE_GROUP_OPS if not hasattr(getattr(engine, "ops", None), m)]
            if missing:
                raise ValueError(f"stream group: wide=True needs an ops backend with the wide entry points; "
                                 f"{type(getattr(engine, 'ops', None)).__name__} lacks {missing}")
        if getattr(engine, "llm_fp8", False):
            missing = [m for m in FP8_GROUP_OPS if not hasattr(getattr(engine, "ops", None), m)]
            if missing:
                raise ValueError(f"stream group: an llm_fp8=True engine needs an ops backend with the lane-batched fp8 entry points; "
                                 f"{type(getattr(engine, 'ops', None)).__name__} lacks {missing}")
            if sampling and not hasattr(engine.ops, "decb_lm_head_sample_fp8"):
                raise ValueError(f"stream group: sampling=True on an llm_fp8=True engine needs an ops backend with the lane-batched fp8 "
                                 f"sampling head; {type(engine.ops).__name__} lacks decb_lm_head_sample_fp8")
        if getattr(engine, "llm_fp4", False):
            missing = [m for m in FP4_GROUP_OPS if not hasattr(getattr(engine, "ops", None), m)]
            if missing:
                raise ValueError(f"stream group: an llm_fp4=True engine needs an ops backend with the lane-batched fp4 entry points and the "
                                 f"lane-batched fp8 head; {type(getattr(engine, 'ops', None)).__name__} lacks {missing}")
            if sampling and not hasattr(engine.ops, "decb_lm_head_sample_fp8"):
                raise ValueError(f"stream group: sampling=True on an llm_fp4=True engine needs an ops backend with the lane-batched fp8 "
                                 f"sampling head; {type(engine.ops).__name__} lacks decb_lm_head_sample_fp8")
        if batched_attn:
            missing = [m for m in ATTN_GROUP_OPS if not hasattr(getattr(engine, "ops", None), m)]
            if missing:
                raise ValueError(f"stream group: batched_attn=True needs an ops backend with the lane-batched attention entry point; "
                                 f"{type(getattr(engine, 'ops', None)).__name__} lacks {missing}")
        if getattr(engine, "decode_tail", False):
            raise ValueError("stream group: decode_tail=True engines are not supported (the persistent layer tail is single-row)")
        self.engine = engine
        self.n_lanes = int(n_lanes)
        self.sampling = bool(sampling)
        self.wide = bool(wide)
        self.batched_attn = bool(batched_attn)
        tc, dev, o = engine.cfg.text, engine.device, engine.ops
        self.lanes: List[SvlmEngine] = [engine] + [
            SvlmEngine(engine.cfg, None, dev, ops=o, max_len=engine.max_len, max_new_tokens=engine.max_new, decode_chunk=engine._fixed_chunk,
                       use_graph=engine.use_graph, kv_slack=engine.kv_slack, kv_page_tokens=engine.kv_page_tokens, decode_tail=False,
                       vit_fp8=engine.vit_fp8, linear_planes=engine.linear_planes, llm_fp8=engine.llm_fp8, share=engine,
                       prefill_fp8=engine.prefill_fp8, llm_fp4=engine.llm_fp4, prefill_fp4=engine.prefill_fp4,
                       prefill_mx=getattr(engine, "prefill_mx", False))
            for _ in range(self.n_lanes - 1)]
        for ln in self.lanes[1:]:
            ln.default_top_k, ln.default_top_p, ln.eos_dev = engine.default_top_k, engine.default_top_p, engine.eos_dev
        B, H, V = self.n_lanes, tc.hidden_size, tc.vocab_size
        self.use_graph = engine.use_graph
        # group-owned activations of the batched step, one row per live lane of the batch
        self.x = torch.zeros((B, H), dtype=BF16, device=dev)
        self.q = torch.zeros((B, engine.qd), dtype=BF16, device=dev)
        self.attn = torch.zeros((B, engine.qd), dtype=BF16, device=dev)
        self.h = torch.zeros((B, tc.intermediate_size), dtype=BF16, device=dev)
        self.logits = torch.zeros((B, V), dtype=torch.float32, device=dev)
        self.ws = o.decb_sampling_ws(V, B, dev)
        eos = list(engine.cfg.eos_token_ids)
        if len(eos) > 8:
            raise ValueError("stream group: at most 8 EOS ids can be suppressed")
        self.suppress = torch.tensor(eos + [-1] * (8 - len(eos)), dtype=torch.int32, device=dev)
        # the lane table (svlm_lane records): rows [0, B) are the batch, written at the start of every generate(); a lane parked by an
        # EOS look gets its row rewritten (limit 0) from the second half of the page-locked staging block
        W = o.LANE_WORDS
        self.table = torch.zeros((B, W), dtype=torch.int64, device=dev)
        self._table_host = torch.zeros((2 * B, W), dtype=torch.int64)
        if dev.type == "cuda":
            self._table_host = self._table_host.pin_memory()
        # the sampling table (svlm_lane_sample records), parallel to the lane table: row j belongs to lane-table row j
        self.samples = self._samples_host = None
        if self.sampling:
            self.samples = torch.zeros((B, o.SAMPLE_WORDS), dtype=torch.int64, device=dev)
            self._samples_host = torch.zeros((B, o.SAMPLE_WORDS), dtype=torch.int64)
            if dev.type == "cuda":
                self._samples_host = self._samples_host.pin_memory()
        # the attention table (svlm_lane_attn records), parallel to the lane table: row j holds the rope table, lin_state, workspace and
        # the (attn_len, chunk) lane-table row j's generate() call picked; `_attn_host_args` keeps the same per lane for the launcher
        self.attn_table = self._attn_table_host = None
        self._attn_host_args = ([], [], [])
        if self.batched_attn:
            self.attn_table = torch.zeros((B, o.ATTN_WORDS), dtype=torch.int64, device=dev)
            self._attn_table_host = torch.zeros((B, o.ATTN_WORDS), dtype=torch.int64)
            if dev.type == "cuda":
                self._attn_table_host = self._attn_table_host.pin_memory()
        if self.wide and dev.type == "cuda" and hasattr(o, "decw_reserve_lds"):
            o.decw_reserve_lds()                 # (before any step is captured into a graph)
        self._graphs = {}
        self.max_graphs = engine.max_graphs
        self._rv = LaneRendezvous(self.n_lanes, lambda reqs: self.generate(reqs, return_exceptions=True))
        self.attach, self.detach, self.submit = self._rv.attach, self._rv.detach, self._rv.submit

    def lane_model(self, i: int) -> LaneModel:
        return LaneModel(self, i)

    # ------------------------------------------------------------------ lane table
    def _record(self, lane: SvlmEngine, cache, limit: int):
        lin = cache.lin_args() if hasattr(cache, "lin_args") else None
        return self.engine.ops.lane_record(cache.pool, None if lin is None else lin[0], cache.slot_of_dev, lane.state, lane.tok_buf,
                                           lane.seen if lane._penalty != 1.0 else None, limit, lane._penalty,
                                           len(self.engine.cfg.eos_token_ids) if lane._suppress is not None else 0)

    def _write_row(self, row: int, rec: np.ndarray, stage_row: int):
        self._table_host[stage_row].copy_(torch.from_numpy(rec))
        self.table[row].copy_(self._table_host[stage_row], non_blocking=True)

    def _sample_record(self, lane: SvlmEngine):
        """The lane's svlm_lane_sample record from what its `generate_begin` left: `_sampling` (None = greedy) and the seed in `rng_dev`."""
        if lane._sampling is None:
            return self.engine.ops.lane_sample_record()
        t, k, p = lane._sampling
        return self.engine.ops.lane_sample_record(lane.rng_dev, t, k, p)

    def _write_sample_row(self, row: int, rec: np.ndarray):
        self._samples_host[row].copy_(torch.from_numpy(rec))
        self.samples[row].copy_(self._samples_host[row], non_blocking=True)

    def _attn_record(self, lane: SvlmEngine, cache):
        """The lane's svlm_lane_attn record from what its `generate_begin` left: the rope table, the workspace, `_attn_len`, `decode_chunk`."""
        lin = cache.lin_args() if hasattr(cache, "lin_args") else None
        return self.engine.ops.lane_attn_record(lane.rope_cs, None if lin is None else lin[1], lane.d_ws, lane._attn_len, lane.decode_chunk,
                                                self.engine.cfg.text.num_heads, slot_of=cache.slot_of_dev, lin=None if lin is None else lin[0])

    def _write_attn_row(self, row: int, rec: np.ndarray):
        self._attn_table_host[row].copy_(torch.from_numpy(rec))
        self.attn_table[row].copy_(self._attn_table_host[row], non_blocking=True)

    def _attn(self, act, tab, B, li, scale):
        """The decode attention of layer `li` for the batch: the single-stream kernel pair once per lane on the same stream (no forked
        branches), or with `batched_attn` all lanes in one `decb_attn` (one split and one combine launch)."""
        e, o, tc = self.engine, self.engine.ops, self.engine.cfg.text
        if getattr(self, "batched_attn", False):      # (getattr: the host tests build group objects with __new__, without the attribute)
            lens, chunks, has_lin = self._attn_host_args
            o.decb_attn(tab, self.attn_table, B, self.q, self.attn, li, tc.num_heads, scale, lens, chunks, has_lin, e.kd // tc.head_dim,
                        tc.head_dim)
            return
        for j, (lane, c) in enumerate(act):
            o.decode_attn(self.q[j], c.pool, li, c.slot_of_dev, lane.rope_cs, self.attn[j], lane.d_ws, tc.num_heads, lane._attn_len,
                          lane.decode_chunk, scale, length=1, len_dev=lane.state[0:1], lin=c.lin_args() if hasattr(c, "lin_args") else None)

    # ------------------------------------------------------------------ one batched decode step
    def _head(self, tab, B, sampled: bool):
        """The head and the token feedback.  `sampled`: some lane of the batch draws its token -- the head adds the Gumbel noise where a
        lane's record asks for it and the finish branches on each lane's mode; an all-greedy batch keeps the greedy pair."""
        e, o, w, tc = self.engine, self.engine.ops, self.engine.w, self.engine.cfg.text
        head_fp8 = e.llm_fp8 or getattr(e, "llm_fp4", False)         # the lm_head is e4m3 in both
        if not sampled:
            if head_fp8:
                o.decb_lm_head_fp8(tab, B, self.x, w.final_norm, tc.rms_eps, w.lm_head8, w.lm_head_s, self.logits, self.suppress, self.ws)
            else:
                o.decb_lm_head(tab, B, self.x, w.final_norm, tc.rms_eps, w.lm_head, self.logits, self.suppress, self.ws)
            o.decb_argmax_finish(tab, B, self.ws, tc.vocab_size, 1)
            return
        if head_fp8:
            o.decb_lm_head_sample_fp8(tab, self.samples, B, self.x, w.final_norm, tc.rms_eps, w.lm_head8, w.lm_head_s, self.logits, self.suppress,
                                      self.ws)
        else:
            o.decb_lm_head_sample(tab, self.samples, B, self.x, w.final_norm, tc.rms_eps, w.lm_head, self.logits, self.suppress, self.ws)
        o.decb_sample_finish(tab, self.samples, B, self.logits, self.suppress, self.ws, tc.vocab_size, 1)

    def _step_launch(self, act, sampled: bool = False):
        """One token for every live lane of the batch: per layer [norm+QKV+append]xB-in-one, B x [attn split, attn combine] (`_attn`),
        [o+res]xB-in-one, [norm+gate/up+SwiGLU]xB-in-one, [down+res]xB-in-one; then the head and the token feedback."""
        e, o, w, tc = self.engine, self.engine.ops, self.engine.w, self.engine.cfg.text
        B, qd, kd, nl = len(act), e.qd, e.kd, len(self.engine.w.layers)
        scale = 1.0 / math.sqrt(tc.head_dim)
        tab = self.table
        if getattr(self, "wide", False):
            self._step_wide(act, tab, B, scale)
            return
        o.decb_embed(tab, B, w.embed, self.x)
        if e.llm_fp8:
            self._layers_fp8(act, tab, B, scale)
            self._head(tab, B, sampled)
            return
        if getattr(e, "llm_fp4", False):
            self._layers_fp4(act, tab, B, scale)
            self._head(tab, B, sampled)
            return
        for li, lw in enumerate(w.layers):
            o.decb_qkv(tab, B, self.x, lw["ln1"], tc.rms_eps, lw["qkv_w"], lw["qkv_b"], self.q, li, qd, kd, tc.head_dim, nl)
            self._attn(act, tab, B, li, scale)
            o.decb_gemv(tab, B, self.attn, lw["o_w"], self.x, self.x)
            o.decb_gate_up(tab, B, self.x, lw["ln2"], tc.rms_eps, lw["gu_w"], self.h)
            o.decb_gemv(tab, B, self.h, lw["down_w"], self.x, self.x)
        self._head(tab, B, sampled)

    def _step_wide(self, act, tab, B, scale):
        """`_step_launch` of a wide group: the same launches with the weight kernels on the MFMA (csrc/decode_wide.hip); greedy head."""
        e, o, w, tc = self.engine, self.engine.ops, self.engine.w, self.engine.cfg.text
        qd, kd, nl = e.qd, e.kd, len(w.layers)
        o.decw_embed(tab, B, w.embed, self.x)
        for li, lw in enumerate(w.layers):
            o.decw_qkv(tab, B, self.x, lw["ln1"], tc.rms_eps, lw["qkv_w"], lw["qkv_b"], self.q, li, qd, kd, tc.head_dim, nl)
            self._attn(act, tab, B, li, scale)
            o.decw_gemv(tab, B, self.attn, lw["o_w"], self.x, self.x)
            o.decw_gate_up(tab, B, self.x, lw["ln2"], tc.rms_eps, lw["gu_w"], self.h)
            o.decw_gemv(tab, B, self.h, lw["down_w"], self.x, self.x)
        o.decw_lm_head(tab, B, self.x, w.final_norm, tc.rms_eps, w.lm_head, self.logits, self.suppress, self.ws)
        o.decw_argmax_finish(tab, B, self.ws, tc.vocab_size, 1)

    def _layers_fp8(self, act, tab, B, scale):
        """The layers of `_step_launch` on e4m3 weights: the same launches with the weight-streaming kernels replaced by their fp8 twins
        (csrc/decode_batch_fp8.hip)."""
        e, o, w, tc = self.engine, self.engine.ops, self.engine.w, self.engine.cfg.text
        qd, kd, nl = e.qd, e.kd, len(w.layers)
        for li, lw in enumerate(w.layers):
            o.decb_qkv_fp8(tab, B, self.x, lw["ln1"], tc.rms_eps, lw["qkv_w8"], lw["qkv_w_s"], lw["qkv_b"], self.q, li, qd, kd, tc.head_dim, nl)
            self._attn(act, tab, B, li, scale)
            o.decb_gemv_fp8(tab, B, self.attn, lw["o_w8"], lw["o_w_s"], self.x, self.x)
            o.decb_gate_up_fp8(tab, B, self.x, lw["ln2"], tc.rms_eps, lw["gu_w8"], lw["gu_w_s"], self.h)
            o.decb_gemv_fp8(tab, B, self.h, lw["down_w8"], lw["down_w_s"], self.x, self.x)

    def _layers_fp4(self, act, tab, B, scale):
        """The layers of `_step_launch` on MXFP4 weights: `_layers_fp8` with the weight-streaming kernels replaced by their fp4 twins
        (csrc/decode_batch_fp4.hip) on the e2m1 codes and e8m0 block scales."""
        e, o, w, tc = self.engine, self.engine.ops, self.engine.w, self.engine.cfg.text
        qd, kd, nl = e.qd, e.kd, len(w.layers)
        for li, lw in enumerate(w.layers):
            o.decb_qkv_fp4(tab, B, self.x, lw["ln1"], tc.rms_eps, lw["qkv_w4"], lw["qkv_w_s4"], lw["qkv_b"], self.q, li, qd, kd, tc.head_dim, nl)
            self._attn(act, tab, B, li, scale)
            o.decb_gemv_fp4(tab, B, self.attn, lw["o_w4"], lw["o_w_s4"], self.x, self.x)
            o.decb_gate_up_fp4(tab, B, self.x, lw["ln2"], tc.rms_eps, lw["gu_w4"], lw["gu_w_s4"], self.h)
            o.decb_gemv_fp4(tab, B, self.h, lw["down_w4"], lw["down_w_s4"], self.x, self.x)

    def _step(self, idx, act, sampled: bool = False):
        if not self.use_graph:
            self._step_launch(act, sampled)
            return
        # keyed on the lanes of the batch, their caches and attention geometry, and on whether the step ends in the sampling pair (the
        # one thing about token choice that changes the launches); penalty / suppression / limits live in the lane table, and each
        # lane's mode, temperature, k, p and seed pointer in the sampling table
        key = tuple((i, c.serial, lane.decode_chunk, lane._attn_len) for i, (lane, c) in zip(idx, act)) + (sampled,)
        hit = self._graphs.get(key)
        if hit is not None and any(r() is not c for r, (_, c) in zip(hit[1], act)):
            hit = None
        if hit is None:
            g = torch.cuda.CUDAGraph()
            # thread-local capture: other lanes' host threads may be preparing their next chunk (frame ingest) meanwhile
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._step_launch(act, sampled)
            for k in [k for k, v in self._graphs.items() if any(r() is None for r in v[1])]:
                del self._graphs[k]          # graphs of pools that are gone (a graph must not keep its pools alive)
            if len(self._graphs) >= self.max_graphs:
                self._graphs.pop(next(iter(self._graphs)))
            hit = self._graphs[key] = (g, [weakref.ref(c) for _, c in act])
        hit[0].replay()

    # ------------------------------------------------------------------ generate
    def generate(self, requests: Sequence[Optional[dict]], return_exceptions: bool = False) -> List:
        """One request (keyword arguments of `SvlmEngine.generate`: ids, cache, video_grid_thw, ...) or None per lane -> one
        `GenerateOutput` or None per lane.  `return_exceptions`: a lane whose request is refused or whose begin / finish raises gets
        the exception object as its result and the other lanes carry on (default: the first such exception is raised)."""
        if len(requests) != self.n_lanes:
            raise ValueError(f"{len(requests)} requests for {self.n_lanes} lanes")
        out: List = [None] * self.n_lanes
        idx, act, ctxs = [], [], []
        for i, req in enumerate(requests):
            if req is None:
                continue
            try:
                ctx = self.lanes[i].generate_begin(**check_request(req, self.sampling))
            except Exception as e:
                if not return_exceptions:
                    raise
                out[i] = e
                continue
            idx.append(i)
            act.append((self.lanes[i], ctx.cache))
            ctxs.append(ctx)
        B = len(act)
        dev_is_gpu = self.engine.device.type == "cuda"
        batched_attn = getattr(self, "batched_attn", False)      # (as in `_attn`: group objects built without __init__)
        if B:
            for j, ((lane, c), ctx) in enumerate(zip(act, ctxs)):
                self._write_row(j, self._record(lane, c, ctx.max_new_tokens), j)
                if self.sampling:
                    self._write_sample_row(j, self._sample_record(lane))
                if batched_attn:
                    self._write_attn_row(j, self._attn_record(lane, c))
            if batched_attn:
                self._attn_host_args = ([lane._attn_len for lane, _ in act], [lane.decode_chunk for lane, _ in act],
                                        [hasattr(c, "lin_args") and c.lin_args() is not None for _, c in act])
            sampled = self.sampling and any(lane._sampling is not None for lane, _ in act)
            n_steps = max(ctx.max_new_tokens for ctx in ctxs) - 1
            done = [False] * B                   # host view: an EOS was seen among the lane's tokens
            polls = [None] * B                   # per lane: (event, host buffer, token count) of the look still in flight
            for step in range(1, n_steps + 1):
                if not any(step < ctx.max_new_tokens and not done[j] for j, ctx in enumerate(ctxs)):
                    break                        # no lane is live: nothing more to launch
                self._step(idx, act, sampled)
                # the single stream's one-poll-behind EOS look, per lane (engine.generate_steps): a lane whose tokens show an EOS is
                # parked (limit 0 in its table row) for the steps not yet queued; its rows past the EOS are rolled back by its commit
                if dev_is_gpu and step % 4 == 0 and step + 1 < n_steps + 1:
                    for j, ((lane, c), ctx) in enumerate(zip(act, ctxs)):
                        if ctx.suppress_eos or done[j] or step + 1 >= ctx.max_new_tokens:
                            continue
                        if polls[j] is not None:
                            polls[j][0].synchronize()
                            if any(int(t) in self.engine.cfg.eos_token_ids for t in polls[j][1][:polls[j][2]].tolist()):
                                done[j] = True
                                self._write_row(j, self._record(lane, c, 0), self.n_lanes + j)
                                continue
                        k = (step // 4) & 1
                        lane._poll_host[k][:step + 1].copy_(lane.tok_buf[:step + 1], non_blocking=True)
                        lane._poll_ev[k].record()
                        polls[j] = (lane._poll_ev[k], lane._poll_host[k], step + 1)
        for i, (lane, _), ctx in zip(idx, act, ctxs):
            try:
                out[i] = lane.generate_finish(ctx)
            except Exception as e:
                if not return_exceptions:
                    raise
                out[i] = e
        return out
