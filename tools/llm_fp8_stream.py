"""The opt-in fp8 language model (SvlmEngine(llm_fp8=True)) against the bf16 default on the bench streams, one JSON line per run.

    python tools/llm_fp8_stream.py [2b|7b ...] [--steps K] [--warmup W] [--out DIR]

Per model: a bf16 stream run, an fp8 stream run and a per-kernel run, each in its OWN child process, one after the other.
  2b: configs[1] (Qwen2-VL-2B, 448x448 @ 1 fps, sink 4 + window 2048, 20 greedy tokens per chunk)
  7b: configs[2] (Qwen2-VL-7B, 448x448 @ 2 fps, sink 4 + window 4096, 20 greedy tokens per chunk)
A stream run fills the KV window first, then times K chunks as bench.py does (random weights, frames resident in HBM, look-ahead ViT),
and reports frames/s, ms per chunk, the chunk's decode steps (first replay start -> last replay end on the GPU timeline, beside the
look-ahead ViT) and its LLM prefill (the per-layer dequantisation into the scratch layer included).  The kernel run times the five
weight-streaming GEMVs in fp8 and bf16 at the model's shapes over 8 layers of distinct weights, cold (512 MiB written between
replays), as bench.py's roofline pass does; bytes are each form's own weight bytes (+ scales, activations).

`--prefill-fp8`: per model ONE child process builds the bf16 model, the scratch-layer fp8 model and the direct fp8 model
(prefill_fp8=True: the prefill GEMMs read the e4m3 weights, csrc/gemm_wfp8.hip) and runs their streams in alternation, `--repeats` times
each; the record (profiles/llm_fp8_prefill_<model>.json with --out) holds every pass, per form the median and the spread of the repeats
of frames/s, ms per chunk and prefill ms per chunk, and direct - scratch / direct - bf16 prefill ms against that spread."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

MODELS = {"2b": dict(fps=1.0, window=2048), "7b": dict(fps=2.0, window=4096)}
SIZE, SINK, NEW = 448, 4, 20
HBM_PEAK_GBS = 8000.0


def stream_run(model_name, fp8, steps, warmup, prefill_fp8=False, model=None):
    """-> (record, model).  `model`: a model an earlier pass built (its engine's timing wrappers are taken off first)."""
    import torch
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.synthetic import ResidentProcessor, ResidentVideo
    from streaming_vlm_amd.weights import random_state_dict
    torch.set_num_threads(min(torch.get_num_threads(), 8))
    p = MODELS[model_name]
    cfg = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b}[model_name]()
    dev = torch.device("cuda", 0)
    tok_per_frame = (SIZE // 28) ** 2
    chunk_tokens = tok_per_frame + 24 + NEW
    max_len = SINK + p["window"] + 2 * chunk_tokens + 64
    fill = max(0, -(-(SINK + p["window"]) // (tok_per_frame + 19 + NEW)) + 1 - warmup)
    first = fill + warmup
    n_chunks = first + steps + 1
    t_build = time.perf_counter()
    if model is None:
        model = S.StreamingQwen2VL(cfg, random_state_dict(cfg, 0, dev), dev, max_len=max_len, max_new_tokens=NEW, llm_fp8=fp8,
                                   **(dict(prefill_fp8=True) if prefill_fp8 else {}))
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t_build
    eng = model._svlm_engine
    plain = (eng._prefill, eng._decode_step)
    video = ResidentVideo(n_chunks + 1, SIZE, p["fps"], 0, dev)
    sec = {"prefill": [], "decode": []}

    def wrap(name, fn):
        def run(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            r = fn(*a, **k)
            e.record()
            sec[name].append((s, e))
            return r
        return run
    eng._prefill = wrap("prefill", eng._prefill)
    eng._decode_step = wrap("decode", eng._decode_step)
    per_chunk, t = [], {}

    def on_chunk(i):
        if sec["decode"]:
            per_chunk.append((sec["prefill"][0][0], sec["prefill"][-1][1], sec["decode"][0][0], sec["decode"][-1][1], len(sec["decode"])))
        sec["prefill"], sec["decode"] = [], []
        if i == first:
            torch.cuda.synchronize()
            t["n0"] = len(per_chunk)
            t["t0"] = time.perf_counter()
        if i == first + steps:
            torch.cuda.synchronize()
            t["t1"] = time.perf_counter()
            t["n1"] = len(per_chunk)

    counts = []
    S.streaming_inference(model=model, processor=ResidentProcessor(), video=video, model_base="Qwen2", duration=n_chunks, previous_text="",
                          kv_policy="sink_window", sink=SINK, window=p["window"], do_sample=False, max_new_tokens=NEW, suppress_eos=True,
                          quiet=True, token_counts=counts, chunk_callback=on_chunk)
    torch.cuda.synchronize()
    eng._prefill, eng._decode_step = plain
    timed = per_chunk[t["n0"]:t["n1"]]
    ms = lambda a, b: a.elapsed_time(b)
    elapsed = t["t1"] - t["t0"]
    frames = steps * video.frames_per_chunk
    return {"run": "stream", "model": cfg.name, "llm_fp8": fp8, "prefill_fp8": bool(prefill_fp8), "config": f"{SIZE}x{SIZE} @{p['fps']:g}fps, sink {SINK} + window {p['window']}, "
            f"{NEW} greedy tokens/chunk", "steps": steps, "warmup": warmup, "frames_per_sec": round(frames / elapsed, 3),
            "ms_per_chunk": round(1e3 * elapsed / steps, 3),
            "decode_ms_per_chunk": round(sum(ms(c[2], c[3]) for c in timed) / len(timed), 3),
            "decode_steps_per_chunk": timed[0][4] if timed else 0,
            "prefill_ms_per_chunk": round(sum(ms(c[0], c[1]) for c in timed) / len(timed), 3),
            "decode_weight_bytes": eng.w.decode_bytes(), "memory_allocated_GiB": round(torch.cuda.memory_allocated() / 2 ** 30, 2),
            "build_seconds": round(build_s, 1)}, model


def kernel_run(model_name, n_layers=8, reps=5):
    import torch
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.ops import HipOps
    from streaming_vlm_amd.weights import quantize_rows_fp8_pow2
    tc = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b}[model_name]().text
    o, dev = HipOps(), "cuda"
    H, I, V, D = tc.hidden_size, tc.intermediate_size, tc.vocab_size, tc.head_dim
    qd, kd = tc.num_heads * D, tc.num_kv_heads * D
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, sc=0.03: (torch.randn(s, generator=g, device=dev) * sc).to(torch.bfloat16)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    x, ln, h, attn = r(H, sc=1.0), r(H) + 1, r(I, sc=1.0), r(qd, sc=1.0)
    qkv_out = torch.zeros(qd + 2 * kd, dtype=torch.bfloat16, device=dev)
    pool = torch.zeros((n_layers, 2, tc.num_kv_heads, 64, D), dtype=torch.bfloat16, device=dev)
    slot = torch.arange(64, dtype=torch.int32, device=dev)
    ln_dev = torch.tensor([5], dtype=torch.int32, device=dev)
    logits = torch.zeros(V, device=dev)
    ws = o.sampling_ws(V, dev)
    shapes = {"qkv": (qd + 2 * kd, H), "o_proj": (H, qd), "gate_up": (2 * I, H), "down_proj": (H, I), "lm_head": (V, H)}
    res = []
    for name, (N, K) in shapes.items():
        nl = 2 if name == "lm_head" else n_layers
        Ws = [r(N, K) for _ in range(nl)]
        W8s = [quantize_rows_fp8_pow2(w) for w in Ws]
        b = r(N, sc=0.1)
        xin = {"o_proj": attn, "down_proj": h}.get(name, x)
        y = torch.zeros(N, dtype=torch.bfloat16, device=dev)
        call = {
            "qkv": (lambda i: o.dec_qkv(x, ln, 1e-6, Ws[i], b, qkv_out, pool, i, slot, qd, kd, len_dev=ln_dev),
                    lambda i: o.dec_qkv_fp8(x, ln, 1e-6, W8s[i][0], W8s[i][1], b, qkv_out, pool, i, slot, qd, kd, len_dev=ln_dev)),
            "o_proj": (lambda i: o.gemv(xin, Ws[i], residual=y, out=y), lambda i: o.gemv_fp8(xin, W8s[i][0], W8s[i][1], residual=y, out=y)),
            "down_proj": (lambda i: o.gemv(xin, Ws[i], residual=y, out=y), lambda i: o.gemv_fp8(xin, W8s[i][0], W8s[i][1], residual=y, out=y)),
            "gate_up": (lambda i: o.dec_gate_up(x, ln, 1e-6, Ws[i], h), lambda i: o.dec_gate_up_fp8(x, ln, 1e-6, W8s[i][0], W8s[i][1], h)),
            "lm_head": (lambda i: o.dec_lm_head(x, ln, 1e-6, Ws[i], logits, None, 1.0, None, ws),
                        lambda i: o.dec_lm_head_fp8(x, ln, 1e-6, W8s[i][0], W8s[i][1], logits, None, 1.0, None, ws)),
        }[name]
        row = {"kernel": name, "N": N, "K": K}
        for form, fn, wbytes in (("bf16", call[0], 2 * N * K), ("fp8", call[1], N * K + 4 * N)):
            launch = lambda: [fn(i) for i in range(nl)]
            launch()
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr):
                launch()
            tms = []
            for _ in range(reps):
                flush.fill_(1)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                gr.replay()
                e.record()
                torch.cuda.synchronize()
                tms.append(s.elapsed_time(e))
            us = 1e3 * sum(tms) / len(tms) / nl
            nbytes = wbytes + 2 * (K + N)
            row[form] = {"us": round(us, 2), "min_us": round(1e3 * min(tms) / nl, 2), "TBps": round(nbytes / us / 1e6, 2),
                         "of_peak": round(nbytes / us / 1e3 / HBM_PEAK_GBS, 3)}
        row["fp8_vs_bf16_time"] = round(row["fp8"]["us"] / row["bf16"]["us"], 3)
        res.append(row)
        del Ws, W8s
        torch.cuda.empty_cache()
    return {"run": "kernels", "model": model_name, "layers_per_replay": n_layers, "cold": "512 MiB written between replays", "kernels": res}


def prefill_run(model_name, steps, warmup, repeats):
    """bf16, scratch fp8 and direct fp8 streams of one model in ONE process, passes alternating; -> the record lines."""
    import statistics
    forms = {"bf16": dict(fp8=False), "fp8_scratch": dict(fp8=True), "fp8_direct": dict(fp8=True, prefill_fp8=True)}
    models, passes = {}, {k: [] for k in forms}
    for r in range(repeats):
        for name, kw in forms.items():
            rec, models[name] = stream_run(model_name, kw["fp8"], steps, warmup, kw.get("prefill_fp8", False), models.get(name))
            rec.update(run="stream", form=name, repeat=r)
            passes[name].append(rec)
    lines = [p for ps in passes.values() for p in ps]
    summ = {"run": "prefill_summary", "model": model_name, "repeats": repeats}
    for name, ps in passes.items():
        for key in ("frames_per_sec", "ms_per_chunk", "prefill_ms_per_chunk", "decode_ms_per_chunk"):
            v = [p[key] for p in ps]
            summ[f"{name}.{key}"] = {"median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
    pm = lambda n: summ[f"{n}.prefill_ms_per_chunk"]
    summ["prefill_ms_direct_minus_scratch"] = round(pm("fp8_direct")["median"] - pm("fp8_scratch")["median"], 3)
    summ["prefill_ms_direct_minus_bf16"] = round(pm("fp8_direct")["median"] - pm("bf16")["median"], 3)
    summ["prefill_ms_repeat_spread"] = max(pm(n)["spread"] for n in forms)
    return lines + [summ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=["2b", "7b"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None, help="directory: one llm_fp8_<model>.json per model (all of its lines)")
    ap.add_argument("--prefill-fp8", action="store_true", help="bf16, scratch fp8 and direct fp8 (prefill_fp8=True) streams in one process per model")
    ap.add_argument("--repeats", type=int, default=3, help="--prefill-fp8: passes per form (their spread is the noise)")
    ap.add_argument("--child", nargs=2, metavar=("MODEL", "RUN"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, run = args.child
        if run == "prefill":
            for line in prefill_run(m, args.steps, args.warmup, args.repeats):
                print(json.dumps(line), flush=True)
            return
        out = kernel_run(m) if run == "kernels" else stream_run(m, run == "fp8", args.steps, args.warmup)[0]
        print(json.dumps(out), flush=True)
        return
    for m in args.models:
        lines = []
        if args.prefill_fp8:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats",
                                str(args.repeats), "--child", m, "prefill"], capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"{m} prefill: child exited with {p.returncode}")
            lines = [json.loads(l) for l in p.stdout.strip().splitlines() if l.startswith("{")]
            for line in lines:
                print(json.dumps(line), flush=True)
            if args.out:
                os.makedirs(args.out, exist_ok=True)
                with open(os.path.join(args.out, f"llm_fp8_prefill_{m}.json"), "w") as f:
                    json.dump(lines, f, indent=1)
            continue
        for run in ("bf16", "fp8", "kernels"):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--child", m, run],
                               capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"{m} {run}: child exited with {p.returncode}")
            line = json.loads(p.stdout.strip().splitlines()[-1])
            print(json.dumps(line), flush=True)
            lines.append(line)
        if len(lines) == 3:
            lines.append({"run": "summary", "model": m, "fp8_vs_bf16_chunk": round(lines[1]["ms_per_chunk"] / lines[0]["ms_per_chunk"], 3),
                          "fp8_vs_bf16_decode": round(lines[1]["decode_ms_per_chunk"] / lines[0]["decode_ms_per_chunk"], 3),
                          "fp8_prefill_extra_ms": round(lines[1]["prefill_ms_per_chunk"] - lines[0]["prefill_ms_per_chunk"], 3)})
            print(json.dumps(lines[-1]), flush=True)
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            with open(os.path.join(args.out, f"llm_fp8_{m}.json"), "w") as f:
                json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
