"""The opt-in MXFP4 language model (SvlmEngine(llm_fp4=True)) against the bf16 default and the fp8 engine on the bench streams.

    python tools/llm_fp4_stream.py [2b|7b ...] [--steps K] [--warmup W] [--repeats R] [--out DIR] [--no-kernels] [--prefill-fp4 | --prefill-mx]

Per model ONE child process builds the bf16, the fp8 (scratch-layer prefill) and the fp4 model and runs their streams in alternation
(tools/llm_fp8_stream.py:stream_run: the window is filled first, then K chunks are timed as bench.py does), `--repeats` times each.  The
record (profiles/llm_fp4_<model>.json with --out) holds every pass and per form the median and the spread of the repeats of frames/s, ms
per chunk, prefill ms per chunk and microseconds per decode step, the decode weight bytes, and the fp4 - fp8 decode-step difference
against that spread.  A second child times the four weight-streaming layer kernels in bf16, fp8 and fp4 at the model's shapes over 8
layers of distinct weights, cold (512 MiB written between replays), bytes being each form's own weight bytes (+ scales, activations).

`--prefill-fp4`: the alternating set becomes bf16, fp8 with the direct prefill (prefill_fp8=True), fp4 with the scratch-layer prefill and
fp4 with the direct prefill (prefill_fp4=True: the prefill GEMMs read the MXFP4 weights, csrc/gemm_wfp4.hip); no kernel child; the
record goes to profiles/llm_fp4_prefill_<model>.json and its summary holds the direct - scratch prefill difference per chunk against
the largest repeat spread.

`--prefill-mx`: the four passes of --prefill-fp4 plus fp4 with the MX prefill (prefill_mx=True: MXFP8 activations x MXFP4 weights on the
block-scaled MFMA, csrc/gemm_mx.hip; its four quantiser launches per layer are inside its prefill time), same run; the record goes to
profiles/llm_fp4_prefill_mx_<model>.json and its summary holds the MX prefill's difference to each of the four."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import llm_fp8_stream as F8          # noqa: E402  (stream_run, the stream geometry)

FORMS = {"bf16": {}, "fp8": dict(llm_fp8=True), "fp4": dict(llm_fp4=True)}
PREFILL_FORMS = {"bf16": {}, "fp8_direct": dict(llm_fp8=True, prefill_fp8=True), "fp4": dict(llm_fp4=True),
                 "fp4_direct": dict(llm_fp4=True, prefill_fp4=True)}
MX_FORMS = dict(PREFILL_FORMS, fp4_mx=dict(llm_fp4=True, prefill_mx=True))


def build(model_name, **kw):
    import torch
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    p = F8.MODELS[model_name]
    cfg = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b}[model_name]()
    dev = torch.device("cuda", 0)
    chunk_tokens = (F8.SIZE // 28) ** 2 + 24 + F8.NEW
    max_len = F8.SINK + p["window"] + 2 * chunk_tokens + 64          # stream_run's own sizing
    return S.StreamingQwen2VL(cfg, random_state_dict(cfg, 0, dev), dev, max_len=max_len, max_new_tokens=F8.NEW, **kw)


def stream_runs(model_name, steps, warmup, repeats, prefill_fp4=False, prefill_mx=False):
    FORMS = MX_FORMS if prefill_mx else PREFILL_FORMS if prefill_fp4 else globals()["FORMS"]
    prefill_fp4 = prefill_fp4 or prefill_mx
    models = {name: build(model_name, **kw) for name, kw in FORMS.items()}
    passes = {k: [] for k in FORMS}
    for r in range(repeats):
        for name in FORMS:
            rec, _ = F8.stream_run(model_name, name.startswith("fp8"), steps, warmup, model=models[name])
            rec.update(form=name, repeat=r, llm_fp4=name.startswith("fp4"), prefill_fp4=name == "fp4_direct", prefill_fp8=name == "fp8_direct", prefill_mx=name == "fp4_mx",
                       decode_us_per_step=round(1e3 * rec["decode_ms_per_chunk"] / max(rec["decode_steps_per_chunk"], 1), 2))
            del rec["build_seconds"]
            passes[name].append(rec)
    lines = [p for ps in passes.values() for p in ps]
    summ = {"run": "fp4_summary", "model": model_name, "repeats": repeats}
    for name, ps in passes.items():
        for key in ("frames_per_sec", "ms_per_chunk", "prefill_ms_per_chunk", "decode_us_per_step"):
            v = [p[key] for p in ps]
            summ[f"{name}.{key}"] = {"median": round(statistics.median(v), 3), "spread": round(max(v) - min(v), 3)}
        summ[f"{name}.decode_weight_bytes"] = ps[0]["decode_weight_bytes"]
    if prefill_fp4:
        pf = lambda n: summ[f"{n}.prefill_ms_per_chunk"]
        summ["run"] = "fp4_prefill_summary"
        summ["prefill_ms_direct_minus_scratch"] = round(pf("fp4_direct")["median"] - pf("fp4")["median"], 3)
        summ["prefill_ms_direct_minus_bf16"] = round(pf("fp4_direct")["median"] - pf("bf16")["median"], 3)
        summ["prefill_ms_direct_minus_fp8_direct"] = round(pf("fp4_direct")["median"] - pf("fp8_direct")["median"], 3)
        summ["prefill_ms_repeat_spread"] = max(pf(n)["spread"] for n in FORMS)
        summ["scratch_layer_allocated"] = {n: models[n]._svlm_engine._fp8_scratch is not None for n in FORMS}
        if prefill_mx:
            summ["run"] = "fp4_prefill_mx_summary"
            for n in PREFILL_FORMS:
                summ[f"prefill_ms_mx_minus_{n}"] = round(pf("fp4_mx")["median"] - pf(n)["median"], 3)
            summ["quantiser_launches_per_prefill"] = 4 * len(models["fp4_mx"]._svlm_engine.w.layers)
        return lines + [summ]
    du = lambda n: summ[f"{n}.decode_us_per_step"]
    summ["decode_us_fp4_minus_fp8"] = round(du("fp4")["median"] - du("fp8")["median"], 2)
    summ["decode_us_fp4_minus_bf16"] = round(du("fp4")["median"] - du("bf16")["median"], 2)
    summ["decode_us_repeat_spread"] = max(du(n)["spread"] for n in FORMS)
    summ["prefill_ms_fp4_minus_fp8"] = round(summ["fp4.prefill_ms_per_chunk"]["median"] - summ["fp8.prefill_ms_per_chunk"]["median"], 3)
    return lines + [summ]


def kernel_run(model_name, n_layers=8, reps=5):
    import torch
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.ops import HipOps
    from streaming_vlm_amd.weights import quantize_blocks_mxfp4, quantize_rows_fp8_pow2
    tc = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b}[model_name]().text
    o, dev = HipOps(), "cuda"
    H, I, D = tc.hidden_size, tc.intermediate_size, tc.head_dim
    qd, kd = tc.num_heads * D, tc.num_kv_heads * D
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, sc=0.03: (torch.randn(s, generator=g, device=dev) * sc).to(torch.bfloat16)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    x, ln, h, attn = r(H, sc=1.0), r(H) + 1, r(I, sc=1.0), r(qd, sc=1.0)
    qkv_out = torch.zeros(qd + 2 * kd, dtype=torch.bfloat16, device=dev)
    pool = torch.zeros((n_layers, 2, tc.num_kv_heads, 64, D), dtype=torch.bfloat16, device=dev)
    slot = torch.arange(64, dtype=torch.int32, device=dev)
    ln_dev = torch.tensor([5], dtype=torch.int32, device=dev)
    shapes = {"qkv": (qd + 2 * kd, H), "o_proj": (H, qd), "gate_up": (2 * I, H), "down_proj": (H, I)}
    res = []
    for name, (N, K) in shapes.items():
        Ws = [r(N, K) for _ in range(n_layers)]
        W8 = [quantize_rows_fp8_pow2(w) for w in Ws]
        W4 = [quantize_blocks_mxfp4(w) for w in Ws]
        b = r(N, sc=0.1)
        xin = {"o_proj": attn, "down_proj": h}.get(name, x)
        y = torch.zeros(N, dtype=torch.bfloat16, device=dev)
        call = {
            "qkv": (lambda i: o.dec_qkv(x, ln, 1e-6, Ws[i], b, qkv_out, pool, i, slot, qd, kd, len_dev=ln_dev),
                    lambda i: o.dec_qkv_fp8(x, ln, 1e-6, *W8[i], b, qkv_out, pool, i, slot, qd, kd, len_dev=ln_dev),
                    lambda i: o.dec_qkv_fp4(x, ln, 1e-6, *W4[i], b, qkv_out, pool, i, slot, qd, kd, len_dev=ln_dev)),
            "gate_up": (lambda i: o.dec_gate_up(x, ln, 1e-6, Ws[i], h), lambda i: o.dec_gate_up_fp8(x, ln, 1e-6, *W8[i], h),
                        lambda i: o.dec_gate_up_fp4(x, ln, 1e-6, *W4[i], h)),
        }.get(name, (lambda i: o.gemv(xin, Ws[i], residual=y, out=y), lambda i: o.gemv_fp8(xin, *W8[i], residual=y, out=y),
                     lambda i: o.gemv_fp4(xin, *W4[i], residual=y, out=y)))
        row = {"kernel": name, "N": N, "K": K}
        for form, fn, wbytes in (("bf16", call[0], 2 * N * K), ("fp8", call[1], N * K + 4 * N), ("fp4", call[2], N * K // 2 + N * K // 32)):
            launch = lambda: [fn(i) for i in range(n_layers)]
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
            us = 1e3 * statistics.median(tms) / n_layers
            nbytes = wbytes + 2 * (K + N)
            row[form] = {"us": round(us, 2), "min_us": round(1e3 * min(tms) / n_layers, 2), "max_us": round(1e3 * max(tms) / n_layers, 2),
                         "TBps": round(nbytes / us / 1e6, 2), "of_peak": round(nbytes / us / 1e3 / F8.HBM_PEAK_GBS, 3)}
        row["fp4_vs_fp8_time"] = round(row["fp4"]["us"] / row["fp8"]["us"], 3)
        row["fp4_vs_bf16_time"] = round(row["fp4"]["us"] / row["bf16"]["us"], 3)
        res.append(row)
        del Ws, W8, W4
        torch.cuda.empty_cache()
    return {"run": "kernels", "model": model_name, "layers_per_replay": n_layers, "cold": "512 MiB written between replays",
            "figure": f"median of {reps} replays", "kernels": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=["2b", "7b"])
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3, help="passes per form (their spread is the noise)")
    ap.add_argument("--out", default=None, help="directory: one llm_fp4_<model>.json per model (all of its lines)")
    ap.add_argument("--no-kernels", action="store_true", help="skip the per-kernel child")
    ap.add_argument("--prefill-fp4", action="store_true", help="bf16, direct fp8, scratch fp4 and direct fp4 (prefill_fp4=True) streams")
    ap.add_argument("--prefill-mx", action="store_true", help="the --prefill-fp4 passes plus fp4 with the MX prefill (prefill_mx=True)")
    ap.add_argument("--child", nargs=2, metavar=("MODEL", "RUN"), default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        m, run = args.child
        for line in ([kernel_run(m)] if run == "kernels" else stream_runs(m, args.steps, args.warmup, args.repeats, args.prefill_fp4, args.prefill_mx)):
            print(json.dumps(line), flush=True)
        return
    for m in args.models:
        lines = []
        for run in ("streams",) + (() if args.no_kernels or args.prefill_fp4 or args.prefill_mx else ("kernels",)):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--warmup", str(args.warmup), "--repeats",
                                str(args.repeats), *(["--prefill-fp4"] if args.prefill_fp4 else []), *(["--prefill-mx"] if args.prefill_mx else []), "--child", m, run],
                               capture_output=True, text=True)
            if p.returncode != 0:
                sys.stderr.write(p.stderr[-4000:])
                raise SystemExit(f"{m} {run}: child exited with {p.returncode}")
            new = [json.loads(l) for l in p.stdout.strip().splitlines() if l.startswith("{")]
            for line in new:
                print(json.dumps(line), flush=True)
            lines += new
        if args.out:
            os.makedirs(args.out, exist_ok=True)
            fname = f"llm_fp4_prefill_mx_{m}.json" if args.prefill_mx else f"llm_fp4_prefill_{m}.json" if args.prefill_fp4 else f"llm_fp4_{m}.json"
            with open(os.path.join(args.out, fname), "w") as f:
                json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
