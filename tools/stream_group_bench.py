"""Stream groups against the single stream, in ONE process and ONE run (BASELINE configs[1] workload: Qwen2-VL-2B widths, 448x448 at
1 fps, window 2048, 20 greedy tokens per chunk, frames resident in HBM; `--model 7b --fps 2 --window 4096` for configs[2]).

Passes, each after its own warm-up (KV window filled, graphs captured), each timed between device syncs:
  solo x REPEATS   the plain engine through streaming_inference, look-ahead ViT off (a group runs strict-causal: same schedule);
                   the spread of the repeats is the run-to-run noise the group figures are read against
  solo_lookahead   the plain engine as bench.py runs it (look-ahead ViT on), for reference
  group B=1..4     B streams through streaming_inference_group on one StreamGroup
and, per B, the decode steps alone: `--steps`-fold replay of the captured batched step (19 steps = one chunk's decode) against the
single-stream step graph.

Kernel averages: run this script under `rocprofv3 --kernel-trace --stats -- python tools/stream_group_bench.py --kernels-only`
(a run of its own, no counters) and pass the stats CSV with --kernel-stats to have the decb_* / single-row averages folded in.

    python tools/stream_group_bench.py --out profiles/stream_group_2b.json
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import streaming_vlm_amd as S  # noqa: E402
from streaming_vlm_amd import config as C  # noqa: E402
from streaming_vlm_amd.stream_group import StreamGroup  # noqa: E402
from streaming_vlm_amd.synthetic import ResidentProcessor, ResidentVideo  # noqa: E402
from streaming_vlm_amd.weights import random_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="2b", choices=["2b", "7b", "tiny"])
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--fps", type=float, default=1.0)
    ap.add_argument("--sink", type=int, default=4)
    ap.add_argument("--window", type=int, default=2048)
    ap.add_argument("--new-tokens", type=int, default=20)
    ap.add_argument("--steps", type=int, default=40, help="timed chunks per pass")
    ap.add_argument("--repeats", type=int, default=3, help="single-stream passes (noise estimate)")
    ap.add_argument("--max-lanes", type=int, default=4)
    ap.add_argument("--kernels-only", action="store_true", help="one short pass per B and nothing else (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats CSV of a --kernels-only run")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    cfg = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b, "tiny": C.tiny}[args.model]()
    tok_per_frame = (args.size // 28) ** 2
    chunk_tokens = tok_per_frame + 24 + args.new_tokens
    max_len = args.sink + args.window + 2 * chunk_tokens + 64
    fill = -(-(args.sink + args.window) // (tok_per_frame + 19 + args.new_tokens)) + 2
    steps = 6 if args.kernels_only else args.steps
    n_chunks = fill + steps
    model = S.StreamingQwen2VL(cfg, random_state_dict(cfg, 0, dev), dev, max_len=max_len, max_new_tokens=args.new_tokens)
    eng = model._svlm_engine
    base = "Qwen2"
    torch.set_num_threads(min(torch.get_num_threads(), 8))

    def stream_kw(seed):
        video = ResidentVideo(n_chunks + 1, args.size, args.fps, seed, dev)
        return dict(video=video, model_base=base, duration=n_chunks, previous_text="", kv_policy="sink_window", sink=args.sink,
                    window=args.window, do_sample=False, max_new_tokens=args.new_tokens, suppress_eos=True, quiet=True)

    def timed(run, streams, lookahead):
        """`run(streams, callbacks)`; the clock runs from the chunk `fill` of stream 0 (every stream has then filled its window: they
        advance in lock-step) to the end; returns ms per chunk-round."""
        t = {}

        def cb(i):
            if i == fill:
                torch.cuda.synchronize()
                t["t0"] = time.perf_counter()
        kws = [dict(stream_kw(s), vision_lookahead=lookahead) for s in range(streams)]
        kws[0]["chunk_callback"] = cb
        counts = [[] for _ in kws]
        for kw, c in zip(kws, counts):
            kw["token_counts"] = c
        run(kws)
        torch.cuda.synchronize()
        ms = 1e3 * (time.perf_counter() - t["t0"]) / steps
        frames = streams * steps * kws[0]["video"].frames_per_chunk
        tokens = sum(sum(c[fill:]) for c in counts)
        return dict(ms_per_chunk=ms, frames_per_sec=frames / (ms * steps / 1e3), tokens_per_sec=tokens / (ms * steps / 1e3), streams=streams)

    def replay_decode(graph, engines, n_dec, rounds=10):
        """ms for `n_dec` replays of a captured decode step, averaged over `rounds`.  Every round starts from the state the chunk's own
        decode started from (its last `n_dec` rows: slots the chunk had reserved), so the replays stay inside rows the cache owns."""
        torch.cuda.synchronize()
        start = [e.state.clone() - n_dec for e in engines]
        total = 0.0
        for r in range(rounds + 1):
            for e, st in zip(engines, start):
                e.state.copy_(st)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_dec):
                graph.replay()
            torch.cuda.synchronize()
            if r:                      # round 0 warms up
                total += time.perf_counter() - t0
        return 1e3 * total / rounds

    proc = ResidentProcessor()
    solo_run = lambda kws: S.streaming_inference(model=model, processor=proc, **kws[0])
    out = dict(model=cfg.name, size=args.size, fps=args.fps, window=args.window, new_tokens=args.new_tokens, timed_chunks=steps,
               note="one process, one run; every pass after its own warm-up; group passes are strict-causal (no look-ahead ViT)")
    if not args.kernels_only:
        solo = [timed(solo_run, 1, False) for _ in range(args.repeats)]
        ms = [p["ms_per_chunk"] for p in solo]
        out["solo"] = dict(passes=solo, ms_per_chunk_median=statistics.median(ms), ms_per_chunk_spread=max(ms) - min(ms),
                           frames_per_sec_median=statistics.median(p["frames_per_sec"] for p in solo))
        out["solo_lookahead"] = timed(solo_run, 1, True)
        out["solo"]["decode_ms_per_chunk"] = replay_decode(eng._graph, [eng], args.new_tokens - 1)       # (its cache is still eng._last_cache)
    groups = {}
    for B in range(1, args.max_lanes + 1):
        group = StreamGroup(eng, B)
        rec = timed(lambda kws: S.streaming_inference_group(model, proc, kws, group=group), B, False)
        # the decode steps alone: the batched step graph of the last batch, one chunk's worth of replays per round
        rec["decode_ms_per_chunk"] = replay_decode(next(reversed(group._graphs.values()))[0], group.lanes, args.new_tokens - 1)
        rec["decode_us_per_step"] = 1e3 * rec["decode_ms_per_chunk"] / (args.new_tokens - 1)
        groups[str(B)] = rec
        del group
    out["group"] = groups
    if "solo" in out:
        ref = out["solo"]["frames_per_sec_median"]
        for B, rec in groups.items():
            rec["aggregate_frames_per_sec_vs_solo"] = rec["frames_per_sec"] / ref
    if args.kernel_stats:
        rows = {}
        for r in csv.DictReader(open(args.kernel_stats)):
            name = r.get("Name") or r.get("KernelName") or ""
            if any(k in name for k in ("decb_", "dec_qkv_kernel", "dec_gate_up_kernel", "dec_lm_head_kernel", "gemv_bf16", "argmax_finish", "decode_attn")):
                rows[name[:120]] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3)
        out["kernel_stats"] = rows
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
