"""Stream groups against the single stream, in ONE process and ONE run (BASELINE configs[1] workload: Qwen2-VL-2B widths, 448x448 at
1 fps, window 2048, 20 greedy tokens per chunk, frames resident in HBM; `--model 7b --fps 2 --window 4096` for configs[2]).

Passes, each after its own warm-up (KV window filled, graphs captured), each timed between device syncs:
  solo x REPEATS   the plain engine through streaming_inference, look-ahead ViT off (a group runs strict-causal: same schedule);
                   the spread of the repeats is the run-to-run noise the group figures are read against
  solo_lookahead   the plain engine as bench.py runs it (look-ahead ViT on), for reference
  group B=1..4     B streams through streaming_inference_group on one StreamGroup
and, per B, the decode steps alone: `--steps`-fold replay of the captured batched step (19 steps = one chunk's decode) against the
single-stream step graph.

`--llm-fp8`: the model is built with llm_fp8=True (e4m3 language-model weights) and takes the same passes through the lane-batched fp8
kernels (csrc/decode_batch_fp8.hip); the bf16 group passes of the same weights run in the same process ("group_bf16"), so the fp8 group
is read against the bf16 group and the solo fp8 stream of ONE run, never against a profile of another day.

`--prefill-fp8` (implies --llm-fp8): the fp8 model is built with prefill_fp8=True -- its prefill GEMMs read the e4m3 weights themselves
(csrc/gemm_wfp8.hip), no dequantisation into a scratch layer -- and the groups of the scratch-layer fp8 model ("group_fp8_scratch") run in
the same process beside the bf16 groups, so direct fp8, scratch fp8 and bf16 groups are all of ONE run.

`--llm-fp4`: the model is built with llm_fp4=True (MXFP4 language-model weights, e4m3 head) and takes the same passes through the
lane-batched fp4 kernels (csrc/decode_batch_fp4.hip); the fp8 groups ("group_fp8") and the bf16 groups ("group_bf16") of the same weights run
in the same process, and per lane count the fp4 decode step is read against the fp8 step of the same run, with the spread of the replay
rounds of both next to it.

`--prefill-fp4` (implies --llm-fp4): the fp4 model is built with prefill_fp4=True (csrc/gemm_wfp4.hip) and the fp8 model it is read
against with prefill_fp8=True: direct fp4, direct fp8 and bf16 groups of ONE run.

`--sample T[,K[,P]]` (may be given more than once): after the greedy passes, the same passes with every stream drawing its tokens
(do_sample=True at temperature T, top_k K -- 0 = off, the default -- and top_p P, a generator seed per stream) through
`StreamGroup(sampling=True)`, and the solo sampled stream of the same run; per setting and B the decode step is read against the greedy
group's step, and the solo sampled step against the solo greedy step (the per-token surcharge of the token choice, once per step in a
group).  Writes profiles/stream_group_sampling_<model>.json.

`--wide [--wide-lanes 1,2,4,8,12,16]`: after the passes above, the same passes through `StreamGroup(wide=True)` (csrc/decode_wide.hip: the
weight kernels on the MFMA) at every lane count of the list ("group_wide"); per lane count the wide decode step is read against the
existing group's step of the SAME run where that group exists (1..4 lanes), with the replay rounds' spread of both beside it.  Writes
profiles/stream_group_wide_<model>.json.  The decw_* kernel averages PER LANE COUNT come from a trace run of its own:
`rocprofv3 --kernel-trace -- python tools/stream_group_bench.py --wide --kernels-only`, whose kernel_trace CSV goes to --kernel-trace
(with --fold): the kernel names do not carry the lane count, so every step's kernels are filed under the lane count its embedding
gather's grid shows.

`--batched-attn` (with or without --wide): every group pass runs twice on the same model, in the same process and run -- the group as it
is (the decode attention once per lane: `2 B n_layers` launches per step) and `StreamGroup(batched_attn=True)` (svlm_decb_attn: one
launch pair per layer) -- `--attn-repeats` times each, alternating; per lane count the record holds the decode step (us, median and
spread of the replay rounds) and the chunk round (ms, median and spread of the repeats) of both, their ratio, and whether the batched
step is below the looped one by more than the two spreads together.  Writes profiles/stream_group_attn_<model>.json.  Per-launch averages
of the batched pair against the single-lane pair come from a trace run of its own (no counters in it):
`rocprofv3 --kernel-trace -- python tools/stream_group_bench.py --wide --batched-attn --kernels-only`, folded in with --kernel-trace
--fold (the attention kernels of a step are filed under its lane count like the decb_* / decw_* kernels).

Kernel averages: run this script under `rocprofv3 --kernel-trace --stats -- python tools/stream_group_bench.py --kernels-only`
(a run of its own, no counters) and pass the stats CSV with --kernel-stats to have the decb_* / single-row averages folded in.

    python tools/stream_group_bench.py --out profiles/stream_group_2b.json
    python tools/stream_group_bench.py --llm-fp8                                      (writes profiles/stream_group_fp8_2b.json)
    python tools/stream_group_bench.py --llm-fp8 --model 7b --fps 2 --window 4096     (writes profiles/stream_group_fp8_7b.json)
    python tools/stream_group_bench.py --prefill-fp8 [--model 7b --fps 2 --window 4096]  (writes profiles/stream_group_prefill_fp8_<model>.json)
    python tools/stream_group_bench.py --llm-fp4                                      (writes profiles/stream_group_fp4_2b.json)
    python tools/stream_group_bench.py --prefill-fp4 [--model 7b --fps 2 --window 4096]  (writes profiles/stream_group_prefill_fp4_<model>.json)
    python tools/stream_group_bench.py --sample 0.9 --sample 0.9,50,1.0               (writes profiles/stream_group_sampling_2b.json)
    python tools/stream_group_bench.py --wide                                         (writes profiles/stream_group_wide_2b.json)
    python tools/stream_group_bench.py --wide --batched-attn                          (writes profiles/stream_group_attn_2b.json)
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


def weight_bytes(kernel, tc):
    """Weight bytes one launch of a lane-batched (decb_*) kernel streams, from its name: e4m3 codes + fp32 row scales for the fp8 twins,
    e2m1 codes + e8m0 block scales for the fp4 twins, bf16 otherwise.  The residual GEMV that splits K over the waves (down_proj) is told from the plain one (o_proj) by its name / KW."""
    import re
    single4 = "decb_" not in kernel and any(k in kernel for k in ("dec_qkv_fp4", "dec_gate_up_fp4", "gemv_fp4"))     # the single-row fp4 twins
    if ("decb_" not in kernel and "decw_" not in kernel and not single4) or "embed" in kernel or "argmax" in kernel:
        return 0
    H, I, qd, kd = tc.hidden_size, tc.intermediate_size, tc.num_heads * tc.head_dim, tc.num_kv_heads * tc.head_dim
    fp8, fp4 = "_fp8" in kernel, "_fp4" in kernel
    if "qkv" in kernel:
        n, k = qd + 2 * kd, H
    elif "gate_up" in kernel:
        n, k = 2 * I, H
    elif "lm_head" in kernel:
        n, k = tc.vocab_size, H
    elif "gemv" in kernel:
        # KW is the third template argument of the lane-batched GEMVs (NB, ROWS, KW, PRE), the second of gemv_fp4_kernel (ROWS, KW, PRE)
        m = re.search(r"<\s*\d+\s*,\s*(\d+)\s*,\s*\d+\s*>", kernel) if single4 else re.search(r"<\s*\d+\s*,\s*\d+\s*,\s*(\d+)\s*,", kernel)
        split = "ksplit" in kernel or ((fp8 or fp4) and m is not None and m.group(1) == "4")
        if "decw_gemv" in kernel:                       # decw_gemv_kernel<KW>: the long K of down_proj takes the 16 waves
            split = "<16>" in kernel
        n, k = (H, I) if split else (H, qd)
    else:
        return 0
    if fp4:
        return n * k // 2 + n * k // 32
    return n * k + 4 * n if fp8 else 2 * n * k


def kernel_stats(path, cfg):
    """The decode kernels' rows of a rocprofv3 kernel_stats CSV: calls, average us and, for the lane-batched GEMVs, TB/s on their weight bytes."""
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r.get("Name") or r.get("KernelName") or ""
        if any(k in name for k in ("decb_", "decw_", "dec_qkv_kernel", "dec_gate_up_kernel", "dec_lm_head_kernel", "gemv_bf16", "argmax_finish", "decode_attn",
                                   "dec_qkv_fp8", "dec_gate_up_fp8", "dec_lm_head_fp8", "gemv_fp8", "dequant_fp8",
                                   "dec_qkv_fp4", "dec_gate_up_fp4", "gemv_fp4", "dequant_fp4")):
            rec = rows[name[:120]] = dict(calls=int(r["Calls"]), avg_us=float(r["AverageNs"]) / 1e3)
            nbytes = weight_bytes(name, cfg.text)
            if nbytes:
                rec["weight_bytes"] = nbytes
                rec["weight_tb_per_s"] = nbytes / (rec["avg_us"] * 1e-6) / 1e12
                rec["weight_gb_per_s"] = 1e3 * rec["weight_tb_per_s"]
    return rows


def kernel_trace_by_lanes(path, cfg):
    """The lane-batched kernels (decb_* / decw_*) of a rocprofv3 kernel_trace CSV, averaged PER LANE COUNT: a step opens with the
    embedding gather, whose grid has one row per lane, and every lane-batched kernel up to the next gather belongs to that step.
    -> {kernel name: {lanes: {calls, avg_us[, weight_gb_per_s]}}}; the wide and the existing group's steps are told apart by their names."""
    rows = list(csv.DictReader(open(path)))
    if not rows:
        return {}
    col = {k.lower(): k for k in rows[0]}
    name_c, t0_c, t1_c = col["kernel_name"], col["start_timestamp"], col["end_timestamp"]
    gy_c, wy_c = col["grid_size_y"], col.get("workgroup_size_y")
    rows.sort(key=lambda r: int(r[t0_c]))
    acc, lanes = {}, None
    for r in rows:
        name = r[name_c]
        if "decb_embed_kernel" in name:
            lanes = int(r[gy_c]) // max(1, int(r[wy_c]) if wy_c else 1)
        if lanes is None or not ("decb_" in name or "decw_" in name or "decode_attn" in name):
            continue
        a = acc.setdefault(name[:120], {}).setdefault(lanes, [0, 0])
        a[0] += 1
        a[1] += int(r[t1_c]) - int(r[t0_c])
    out = {}
    for name, per in acc.items():
        nbytes = weight_bytes(name, cfg.text)
        for lanes, (calls, ns) in sorted(per.items()):
            rec = out.setdefault(name, {})[str(lanes)] = dict(calls=calls, avg_us=ns / calls / 1e3)
            if nbytes:
                rec["weight_gb_per_s"] = nbytes / (rec["avg_us"] * 1e-6) / 1e9
    return out


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
    ap.add_argument("--llm-fp8", action="store_true", help="e4m3 language-model weights: fp8 solo + fp8 groups, and the bf16 groups of the same run")
    ap.add_argument("--prefill-fp8", action="store_true", help="--llm-fp8 with the prefill on the e4m3 weights (prefill_fp8=True); the scratch-layer "
                                                               "fp8 groups and the bf16 groups run in the same process")
    ap.add_argument("--llm-fp4", action="store_true", help="MXFP4 language-model weights: fp4 solo + fp4 groups, and the fp8 and bf16 groups of the same run")
    ap.add_argument("--prefill-fp4", action="store_true", help="--llm-fp4 with the prefill on the MXFP4 weights (prefill_fp4=True); the fp8 groups it is "
                                                               "read against get prefill_fp8=True")
    ap.add_argument("--sample", action="append", default=[], metavar="T[,K[,P]]",
                    help="also run solo and groups with every stream sampling at temperature T, top_k K (0 = off) and top_p P")
    ap.add_argument("--wide", action="store_true", help="also run StreamGroup(wide=True) at every lane count of --wide-lanes, read against the "
                                                        "existing groups of the same run")
    ap.add_argument("--wide-lanes", default="1,2,4,8,12,16", help="lane counts of the --wide passes")
    ap.add_argument("--batched-attn", action="store_true", help="run every group (and --wide group) with and without batched_attn=True, alternating, "
                                                                "and record both")
    ap.add_argument("--attn-repeats", type=int, default=3, help="--batched-attn: timed passes per group and variant")
    ap.add_argument("--kernel-trace", default=None, help="rocprofv3 kernel_trace CSV of a --kernels-only run: lane-batched kernel averages per lane count")
    ap.add_argument("--kernels-only", action="store_true", help="one short pass per B and nothing else (for a rocprofv3 --kernel-trace run)")
    ap.add_argument("--kernel-stats", default=None, help="rocprofv3 kernel_stats CSV of a --kernels-only run")
    ap.add_argument("--fold", default=None, help="with --kernel-stats: add the kernel averages to this earlier record of the same workload "
                                                 "and write it to --out; no GPU work")
    ap.add_argument("--out", default=None, help="record file; --llm-fp8 timed runs default to profiles/stream_group_fp8_<model>.json")
    args = ap.parse_args()
    args.llm_fp8 = args.llm_fp8 or args.prefill_fp8
    args.llm_fp4 = args.llm_fp4 or args.prefill_fp4
    if args.llm_fp4 and args.llm_fp8:
        ap.error("--llm-fp4 / --prefill-fp4 and --llm-fp8 / --prefill-fp8 are two formats of the same matrices: one run, one of them "
                 "(an fp4 run measures the fp8 groups of the same weights itself)")
    settings = []
    for spec in args.sample:
        f = spec.split(",")
        if not 1 <= len(f) <= 3:
            ap.error(f"--sample {spec}: T[,K[,P]]")
        settings.append((float(f[0]), int(f[1]) if len(f) > 1 else 0, float(f[2]) if len(f) > 2 else 1.0))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if settings and not args.kernels_only and not args.fold and args.out is None:
        args.out = os.path.join(root, "profiles", f"stream_group_sampling_{args.model}.json")
    if args.llm_fp8 and not args.kernels_only and not args.fold and args.out is None:
        stem = "stream_group_prefill_fp8" if args.prefill_fp8 else "stream_group_fp8"
        args.out = os.path.join(root, "profiles", f"{stem}_{args.model}.json")

    if args.llm_fp4 and not args.kernels_only and not args.fold and args.out is None:
        stem = "stream_group_prefill_fp4" if args.prefill_fp4 else "stream_group_fp4"
        args.out = os.path.join(root, "profiles", f"{stem}_{args.model}.json")

    wide_lanes = [int(v) for v in args.wide_lanes.split(",")] if args.wide else []
    if args.wide and (args.llm_fp8 or args.llm_fp4 or settings):
        ap.error("--wide is bf16 weights and greedy decoding: not with --llm-fp8 / --llm-fp4 / --sample")
    if (args.wide or args.batched_attn) and not args.kernels_only and not args.fold and args.out is None:
        args.out = os.path.join(root, "profiles", f"stream_group_{'attn' if args.batched_attn else 'wide'}_{args.model}.json")
    if args.batched_attn and (args.llm_fp8 or args.llm_fp4 or settings):
        ap.error("--batched-attn measures the bf16 greedy groups (narrow and --wide); the flag itself combines with every engine")
    cfg = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b, "tiny": C.tiny}[args.model]()
    if args.fold:
        if not args.kernel_stats and not args.kernel_trace:
            ap.error("--fold needs --kernel-stats or --kernel-trace")
        out = json.load(open(args.fold))
        if args.kernel_stats:
            out["kernel_stats"] = kernel_stats(args.kernel_stats, cfg)
        if args.kernel_trace:
            out["kernel_avg_by_lanes"] = kernel_trace_by_lanes(args.kernel_trace, cfg)
        with open(args.out or args.fold, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")
        return
    dev = torch.device("cuda", 0)
    tok_per_frame = (args.size // 28) ** 2
    chunk_tokens = tok_per_frame + 24 + args.new_tokens
    max_len = args.sink + args.window + 2 * chunk_tokens + 64
    fill = -(-(args.sink + args.window) // (tok_per_frame + 19 + args.new_tokens)) + 2
    steps = 6 if args.kernels_only else args.steps
    n_chunks = fill + steps
    sd = random_state_dict(cfg, 0, dev)
    model = S.StreamingQwen2VL(cfg, sd, dev, max_len=max_len, max_new_tokens=args.new_tokens, llm_fp8=args.llm_fp8,
                               **(dict(prefill_fp8=True) if args.prefill_fp8 else {}), **(dict(llm_fp4=True) if args.llm_fp4 else {}),
                               **(dict(prefill_fp4=True) if args.prefill_fp4 else {}))
    eng = model._svlm_engine
    base = "Qwen2"
    torch.set_num_threads(min(torch.get_num_threads(), 8))

    def stream_kw(seed, sample=None):
        video = ResidentVideo(n_chunks + 1, args.size, args.fps, seed, dev)
        kw = dict(video=video, model_base=base, duration=n_chunks, previous_text="", kv_policy="sink_window", sink=args.sink,
                  window=args.window, do_sample=False, max_new_tokens=args.new_tokens, suppress_eos=True, quiet=True)
        if sample is not None:
            kw.update(do_sample=True, temperature=sample[0], top_k=sample[1], top_p=sample[2], generator=torch.Generator().manual_seed(1000 + seed))
        return kw

    def timed(run, streams, lookahead, sample=None):
        """`run(streams, callbacks)`; the clock runs from the chunk `fill` of stream 0 (every stream has then filled its window: they
        advance in lock-step) to the end; returns ms per chunk-round."""
        t = {}

        def cb(i):
            if i == fill:
                torch.cuda.synchronize()
                t["t0"] = time.perf_counter()
        kws = [dict(stream_kw(s, sample), vision_lookahead=lookahead) for s in range(streams)]
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
        replay_decode.rounds_ms = []   # the rounds of the last call: their spread is the noise a step is read against
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
                replay_decode.rounds_ms.append(1e3 * (time.perf_counter() - t0))
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

    if args.kernels_only and args.llm_fp4:
        timed(solo_run, 1, False)      # the single-row fp4 kernels in the same trace, beside their lane-batched twins

    def group_passes(m, sample=None, wide=False):
        groups = {}
        for B in (wide_lanes if wide else range(1, args.max_lanes + 1)):
            group = StreamGroup(m._svlm_engine, B, sampling=sample is not None, **(dict(wide=True) if wide else {}))
            rec = timed(lambda kws: S.streaming_inference_group(m, proc, kws, group=group), B, False, sample)
            # the decode steps alone: the batched step graph of the last batch, one chunk's worth of replays per round
            rec["decode_ms_per_chunk"] = replay_decode(next(reversed(group._graphs.values()))[0], group.lanes, args.new_tokens - 1)
            rec["decode_us_per_step"] = 1e3 * rec["decode_ms_per_chunk"] / (args.new_tokens - 1)
            # the rounds' median and spread beside their mean: one slow round (another process on the machine) moves the mean, not the median
            rec["decode_us_per_step_median"] = 1e3 * statistics.median(replay_decode.rounds_ms) / (args.new_tokens - 1)
            rec["decode_us_per_step_spread"] = 1e3 * (max(replay_decode.rounds_ms) - min(replay_decode.rounds_ms)) / (args.new_tokens - 1)
            groups[str(B)] = rec
            del group
        return groups

    def attn_passes(m, wide=False):
        """Every lane count with and without batched_attn=True: `--attn-repeats` timed passes each, alternating (a drift of the machine hits
        both alike), and the decode step of each from the captured step graph of its last batch.  -> ({B: looped record}, {B: batched record +
        comparison})"""
        reps = 1 if args.kernels_only else max(1, args.attn_repeats)
        looped, cmp_ = {}, {}
        for B in (wide_lanes if wide else range(1, args.max_lanes + 1)):
            pair = {}
            for name, kw in (("looped", {}), ("batched", dict(batched_attn=True))):
                pair[name] = [StreamGroup(m._svlm_engine, B, **kw, **(dict(wide=True) if wide else {})), []]
            # A variant's step graph is replayed RIGHT AFTER that variant's own last pass: lane 0 of both groups is the model's engine, which
            # keeps only its last cache alive (`_last_cache`), so once the other group has run a pass the pools, slot tables and planes this
            # graph's launches address are gone.
            steps_ = {}
            for r in range(reps):
                for name, (group, passes) in pair.items():
                    passes.append(timed(lambda kws, g=group: S.streaming_inference_group(m, proc, kws, group=g), B, False))
                    if r == reps - 1:
                        ms_chunk = replay_decode(next(reversed(group._graphs.values()))[0], group.lanes, args.new_tokens - 1)
                        steps_[name] = (ms_chunk, list(replay_decode.rounds_ms))
            recs = {}
            for name, (group, passes) in pair.items():
                ms = [q["ms_per_chunk"] for q in passes]
                rec = dict(passes[len(passes) // 2], passes_ms_per_chunk=ms, ms_per_chunk_median=statistics.median(ms), ms_per_chunk_spread=max(ms) - min(ms))
                rec["decode_ms_per_chunk"], rounds_ms = steps_[name]
                rec["decode_us_per_step"] = 1e3 * rec["decode_ms_per_chunk"] / (args.new_tokens - 1)
                rec["decode_us_per_step_median"] = 1e3 * statistics.median(rounds_ms) / (args.new_tokens - 1)
                rec["decode_us_per_step_spread"] = 1e3 * (max(rounds_ms) - min(rounds_ms)) / (args.new_tokens - 1)
                recs[name] = rec
            lo, ba = recs["looped"], recs["batched"]
            step_spread = lo["decode_us_per_step_spread"] + ba["decode_us_per_step_spread"]
            round_spread = lo["ms_per_chunk_spread"] + ba["ms_per_chunk_spread"]
            print(f"[batched-attn] {'wide ' if wide else ''}{B} lanes: step {lo['decode_us_per_step_median']:.0f} -> {ba['decode_us_per_step_median']:.0f} us "
                  f"(spreads {step_spread:.0f}), round {lo['ms_per_chunk_median']:.2f} -> {ba['ms_per_chunk_median']:.2f} ms", file=sys.stderr, flush=True)
            looped[str(B)] = lo
            cmp_[str(B)] = dict(batched=ba,                 # (the looped record is the plain group's: `group` / `group_wide` of the file)
                                decode_step_batched_vs_looped=ba["decode_us_per_step_median"] / lo["decode_us_per_step_median"],
                                decode_step_us_saved=lo["decode_us_per_step_median"] - ba["decode_us_per_step_median"],
                                decode_step_spread_of_both_us=step_spread,
                                decode_step_below_by_more_than_spread=lo["decode_us_per_step_median"] - ba["decode_us_per_step_median"] > step_spread,
                                chunk_round_batched_vs_looped=ba["ms_per_chunk_median"] / lo["ms_per_chunk_median"],
                                chunk_round_ms_saved=lo["ms_per_chunk_median"] - ba["ms_per_chunk_median"],
                                chunk_round_spread_of_both_ms=round_spread,
                                chunk_round_below_by_more_than_spread=lo["ms_per_chunk_median"] - ba["ms_per_chunk_median"] > round_spread)
            del pair
        return looped, cmp_

    if args.batched_attn:
        # (the looped side IS the plain group: it is measured once, here)
        groups, narrow_cmp = attn_passes(model)
        out["group"] = groups
        out["batched_attn"] = dict(repeats=args.attn_repeats, group=narrow_cmp)
    else:
        groups = out["group"] = group_passes(model)
    out["llm_fp8"] = bool(args.llm_fp8)
    out["prefill_fp8"] = bool(args.prefill_fp8)
    out["llm_fp4"] = bool(args.llm_fp4)
    out["prefill_fp4"] = bool(args.prefill_fp4)
    out["decode_weight_bytes"] = eng.w.decode_bytes()
    if "solo" in out:
        ref = out["solo"]["frames_per_sec_median"]
        for B, rec in groups.items():
            rec["aggregate_frames_per_sec_vs_solo"] = rec["frames_per_sec"] / ref
    if args.llm_fp8:
        # the bf16 groups of the same weights, same process, same run: what the fp8 groups are read against
        bf = S.StreamingQwen2VL(cfg, sd, dev, max_len=max_len, max_new_tokens=args.new_tokens)
        gb = out["group_bf16"] = group_passes(bf)
        out["decode_weight_bytes_bf16"] = bf._svlm_engine.w.decode_bytes()
        for B, rec in groups.items():
            rec["decode_step_vs_bf16_group"] = rec["decode_us_per_step"] / gb[B]["decode_us_per_step"]
            rec["frames_per_sec_vs_bf16_group"] = rec["frames_per_sec"] / gb[B]["frames_per_sec"]
        del bf
        if args.prefill_fp8:
            # ... and the groups of the scratch-layer fp8 model (dequantisation + bf16 GEMMs per lane prefill), same weights, same run
            sc = S.StreamingQwen2VL(cfg, sd, dev, max_len=max_len, max_new_tokens=args.new_tokens, llm_fp8=True)
            gs = out["group_fp8_scratch"] = group_passes(sc)
            for B, rec in groups.items():
                rec["frames_per_sec_vs_scratch_group"] = rec["frames_per_sec"] / gs[B]["frames_per_sec"]
            del sc
        best = lambda g: max(g, key=lambda B: g[B]["frames_per_sec"])
        out["best"] = dict(fp8_lanes=int(best(groups)), fp8_frames_per_sec=groups[best(groups)]["frames_per_sec"],
                           bf16_lanes=int(best(gb)), bf16_frames_per_sec=gb[best(gb)]["frames_per_sec"])
        if "solo" in out:
            # the only margin: the solo repeats' own spread, as frames/s
            fps_solo = [p["frames_per_sec"] for p in out["solo"]["passes"]]
            out["best"].update(solo_fp8_frames_per_sec=ref, solo_fp8_frames_per_sec_spread=max(fps_solo) - min(fps_solo))
    if args.llm_fp4:
        # the fp8 groups (direct prefill when the fp4 model has one) and the bf16 groups of the same weights, same process, same run
        f8 = S.StreamingQwen2VL(cfg, sd, dev, max_len=max_len, max_new_tokens=args.new_tokens, llm_fp8=True,
                                **(dict(prefill_fp8=True) if args.prefill_fp4 else {}))
        g8 = out["group_fp8"] = group_passes(f8)
        out["decode_weight_bytes_fp8"] = f8._svlm_engine.w.decode_bytes()
        del f8
        bf = S.StreamingQwen2VL(cfg, sd, dev, max_len=max_len, max_new_tokens=args.new_tokens)
        gb = out["group_bf16"] = group_passes(bf)
        out["decode_weight_bytes_bf16"] = bf._svlm_engine.w.decode_bytes()
        del bf
        for B, rec in groups.items():
            rec["decode_step_vs_fp8_group"] = rec["decode_us_per_step_median"] / g8[B]["decode_us_per_step_median"]
            # the replay rounds' spread of both steps, as a fraction of the fp8 step: what the ratio is read against
            rec["decode_step_vs_fp8_group_spread"] = (rec["decode_us_per_step_spread"] + g8[B]["decode_us_per_step_spread"]) / g8[B]["decode_us_per_step_median"]
            rec["frames_per_sec_vs_fp8_group"] = rec["frames_per_sec"] / g8[B]["frames_per_sec"]
            rec["decode_step_vs_bf16_group"] = rec["decode_us_per_step_median"] / gb[B]["decode_us_per_step_median"]
            rec["frames_per_sec_vs_bf16_group"] = rec["frames_per_sec"] / gb[B]["frames_per_sec"]
        best = lambda g: max(g, key=lambda B: g[B]["frames_per_sec"])
        out["best"] = dict(fp4_lanes=int(best(groups)), fp4_frames_per_sec=groups[best(groups)]["frames_per_sec"],
                           fp8_lanes=int(best(g8)), fp8_frames_per_sec=g8[best(g8)]["frames_per_sec"],
                           bf16_lanes=int(best(gb)), bf16_frames_per_sec=gb[best(gb)]["frames_per_sec"])
        if "solo" in out:
            fps_solo = [p["frames_per_sec"] for p in out["solo"]["passes"]]
            out["best"].update(solo_fp4_frames_per_sec=ref, solo_fp4_frames_per_sec_spread=max(fps_solo) - min(fps_solo))
    if args.wide:
        # the wide groups of the same model, same process, same run: read against the existing groups above, never against another day's
        if args.batched_attn:
            gw, out["batched_attn"]["group_wide"] = attn_passes(model, wide=True)
            out["group_wide"] = gw
        else:
            gw = out["group_wide"] = group_passes(model, wide=True)
        for B, rec in gw.items():
            if "solo" in out:
                rec["aggregate_frames_per_sec_vs_solo"] = rec["frames_per_sec"] / ref
            if B in groups:
                g = groups[B]
                rec["decode_step_vs_group"] = rec["decode_us_per_step_median"] / g["decode_us_per_step_median"]
                rec["decode_step_us_saved_vs_group"] = g["decode_us_per_step_median"] - rec["decode_us_per_step_median"]
                rec["decode_step_spread_of_both_us"] = rec["decode_us_per_step_spread"] + g["decode_us_per_step_spread"]
                rec["frames_per_sec_vs_group"] = rec["frames_per_sec"] / g["frames_per_sec"]
        best = lambda g: max(g, key=lambda B: g[B]["frames_per_sec"])
        out["best"] = dict(wide_lanes=int(best(gw)), wide_frames_per_sec=gw[best(gw)]["frames_per_sec"],
                           group_lanes=int(best(groups)), group_frames_per_sec=groups[best(groups)]["frames_per_sec"])
    if settings:
        # every stream draws its tokens: the solo sampled stream and the sampling groups of the same process and run, each read against
        # its greedy counterpart above
        n_dec = args.new_tokens - 1
        out["sampling"] = {}
        for t, k, p in settings:
            rec = out["sampling"][f"T={t:g},top_k={k},top_p={p:g}"] = dict(temperature=t, top_k=k, top_p=p)
            if "solo" in out:
                passes = [timed(solo_run, 1, False, (t, k, p)) for _ in range(args.repeats)]
                fps = [q["frames_per_sec"] for q in passes]
                rec["solo"] = dict(passes=passes, frames_per_sec_median=statistics.median(fps), frames_per_sec_spread=max(fps) - min(fps),
                                   decode_ms_per_chunk=replay_decode(eng._graph, [eng], n_dec))
                rec["solo"]["decode_us_per_step"] = 1e3 * rec["solo"]["decode_ms_per_chunk"] / n_dec
                rec["solo"]["surcharge_us_per_step"] = rec["solo"]["decode_us_per_step"] - 1e3 * out["solo"]["decode_ms_per_chunk"] / n_dec
            rec["group"] = group_passes(model, (t, k, p))
            for B, g in rec["group"].items():
                g["surcharge_us_per_step_vs_greedy_group"] = g["decode_us_per_step"] - groups[B]["decode_us_per_step"]
                g["frames_per_sec_vs_greedy_group"] = g["frames_per_sec"] / groups[B]["frames_per_sec"]
                if "solo" in rec:
                    g["aggregate_frames_per_sec_vs_solo_sampled"] = g["frames_per_sec"] / rec["solo"]["frames_per_sec_median"]
                    g["surcharge_vs_solo_surcharge"] = g["surcharge_us_per_step_vs_greedy_group"] / rec["solo"]["surcharge_us_per_step"]
    if args.kernel_stats:
        out["kernel_stats"] = kernel_stats(args.kernel_stats, cfg)
    if args.kernel_trace:
        out["kernel_avg_by_lanes"] = kernel_trace_by_lanes(args.kernel_trace, cfg)
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
