#!/usr/bin/env python
"""The MX prefill GEMM (svlm_quant_mxfp8 + svlm_gemm_mx_a8w4*, csrc/gemm_mx.hip) against the direct weight-fp4 GEMM, the scratch path and
the plain bf16 GEMM at every prefill shape of a language model, cold weights, the forms ALTERNATING inside one process.

    python tools/gemm_mx_vs_bf16.py [2b] [7b] [--rows 290 590 1024 4096] [--layers 8] [--reps 5] [--out FILE]

The method of tools/gemm_wfp4_vs_bf16.py: per shape `--layers` distinct weight matrices (one graph replay = one launch per matrix, so no
matrix is read twice per replay) and 512 MiB written between replays; `reps` replays per form, interleaved, median, min and max per
launch.  Forms, per GEMM:
    quant      svlm_quant_mxfp8 of the A operand alone
    mx         the MX GEMM alone (A already quantised)
    quant_mx   quantiser + MX GEMM, what a prefill_mx layer pays
    wfp4       the direct weight-fp4 GEMM (bf16 activations)
    dequant    svlm_dequant_fp4_bf16 of the matrix
    bf16       the bf16 GEMM on W'
The comparisons a reader wants: mx vs bf16 at M = 4096 (the scaled MFMA runs e4m3 operands at twice the bf16 rate), quant_mx vs
bf16 + dequant there (the scratch path a prefill_fp4 engine takes above 1024 rows), and quant_mx vs wfp4 at M = 290-590.
`--out profiles/gemm_mx_vs_bf16.json` keeps the record."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from streaming_vlm_amd import config as C  # noqa: E402
from streaming_vlm_amd._lib import ACT_SWIGLU  # noqa: E402
from streaming_vlm_amd.ops import HipOps  # noqa: E402
from streaming_vlm_amd.weights import quantize_blocks_mxfp4  # noqa: E402

BF16 = torch.bfloat16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("models", nargs="*", default=["2b", "7b"])
    ap.add_argument("--rows", type=int, nargs="+", default=[290, 590, 1024, 4096])
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    o, dev = HipOps(), "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s, sc=0.03: (torch.randn(s, generator=g, device=dev) * sc).to(BF16)
    flush = torch.empty(512 << 20, dtype=torch.uint8, device=dev)
    out = []
    forms = ("quant", "mx", "quant_mx", "wfp4", "dequant", "bf16")
    for name in args.models:
        tc = {"2b": C.qwen2_vl_2b, "7b": C.qwen2_vl_7b, "3b": C.qwen2_5_vl_3b}[name]().text
        H, I, D = tc.hidden_size, tc.intermediate_size, tc.head_dim
        qd, kd = tc.num_heads * D, tc.num_kv_heads * D
        # (GEMM, rows of W, K, epilogue): the four calls of SvlmEngine._prefill
        shapes = [("qkv", qd + 2 * kd, H, "bias"), ("o_proj", H, qd, "res+norm"), ("gate_up", 2 * I, H, "swiglu"), ("down_proj", H, I, "res+norm")]
        for M in args.rows:
            for gemm, Nw, K, epi in shapes:
                N = Nw // 2 if epi == "swiglu" else Nw
                nl = args.layers
                W4s = [quantize_blocks_mxfp4(r(Nw, K)) for _ in range(nl)]
                Wb = [torch.empty((Nw, K), dtype=BF16, device=dev) for _ in range(nl)]
                for (q, s), w in zip(W4s, Wb):
                    o.dequant_fp4(q, s, w)
                A, b, nw = r(M, K, sc=1.0), r(Nw, sc=0.1), r(N) + 1
                x, xn, y = r(M, N, sc=1.0), torch.empty((M, N), dtype=BF16, device=dev), torch.empty((M, N), dtype=BF16, device=dev)
                A8, As = o.quant_mxfp8(A)

                def quant(i):
                    o.quant_mxfp8(A, A8, As)

                def mx(i):
                    q, s = W4s[i]
                    if epi == "bias":
                        o.gemm_mx_a8w4(A8, As, q, s, bias=b, out=y)
                    elif epi == "swiglu":
                        o.gemm_mx_a8w4(A8, As, q, s, out=y, act=ACT_SWIGLU)
                    else:
                        o.gemm_mx_a8w4_norm(A8, As, q, s, nw, 1e-6, y, xn, residual=x)

                def quant_mx(i):
                    quant(i)
                    mx(i)

                def wfp4(i):
                    q, s = W4s[i]
                    if epi == "bias":
                        o.gemm_wfp4(A, q, s, bias=b, out=y)
                    elif epi == "swiglu":
                        o.gemm_wfp4(A, q, s, out=y, act=ACT_SWIGLU)
                    else:
                        o.gemm_wfp4_norm(A, q, s, nw, 1e-6, y, xn, residual=x)

                def bf16(i):
                    if epi == "bias":
                        o.gemm(A, Wb[i], bias=b, out=y)
                    elif epi == "swiglu":
                        o.gemm(A, Wb[i], out=y, act=ACT_SWIGLU)
                    else:
                        o.gemm_norm(A, Wb[i], nw, 1e-6, y, xn, residual=x)

                def dequant(i):
                    o.dequant_fp4(W4s[i][0], W4s[i][1], Wb[i])
                fns = dict(quant=quant, mx=mx, quant_mx=quant_mx, wfp4=wfp4, dequant=dequant, bf16=bf16)
                graphs, times = {}, {}
                for form in forms:
                    for i in range(nl):
                        fns[form](i)
                    torch.cuda.synchronize()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr):
                        for i in range(nl):
                            fns[form](i)
                    graphs[form], times[form] = gr, []
                for _ in range(args.reps):
                    for form, gr in graphs.items():
                        flush.fill_(1)
                        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        s.record()
                        gr.replay()
                        e.record()
                        torch.cuda.synchronize()
                        times[form].append(1e3 * s.elapsed_time(e) / nl)
                med = {k: statistics.median(v) for k, v in times.items()}
                row = dict(model=name, M=M, gemm=gemm, N=N, K=K, epilogue=epi, layers_per_replay=nl, reps=args.reps,
                           **{f"{k}_us": round(med[k], 2) for k in med}, **{f"{k}_min_us": round(min(times[k]), 2) for k in times},
                           **{f"{k}_max_us": round(max(times[k]), 2) for k in times},
                           mx_vs_bf16=round(med["mx"] / med["bf16"], 3),
                           quant_mx_vs_bf16_plus_dequant=round(med["quant_mx"] / (med["bf16"] + med["dequant"]), 3),
                           quant_mx_vs_wfp4=round(med["quant_mx"] / med["wfp4"], 3),
                           mx_TFLOPs=round(2.0 * M * Nw * K / med["mx"] / 1e6, 1), bf16_TFLOPs=round(2.0 * M * Nw * K / med["bf16"] / 1e6, 1))
                print(json.dumps(row), flush=True)
                out.append(row)
                del W4s, Wb, graphs
                torch.cuda.empty_cache()
        # per layer: the four GEMMs of a layer summed, per M
        for M in args.rows:
            rows = [x_ for x_ in out if x_["model"] == name and x_.get("gemm") and x_["M"] == M]
            tot = {k: sum(x_[f"{k}_us"] for x_ in rows) for k in forms}
            line = dict(model=name, M=M, layer="sum of the four GEMMs", **{f"{k}_us": round(v, 1) for k, v in tot.items()},
                        mx_vs_bf16=round(tot["mx"] / tot["bf16"], 3),
                        quant_mx_vs_bf16_plus_dequant=round(tot["quant_mx"] / (tot["bf16"] + tot["dequant"]), 3),
                        quant_mx_vs_wfp4=round(tot["quant_mx"] / tot["wfp4"], 3))
            print(json.dumps(line), flush=True)
            out.append(line)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
