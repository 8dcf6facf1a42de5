"""`SvlmEngine(llm_fp4=True, prefill_mx=True)` on the MI355X, end to end: MXFP8 activations x MXFP4 weights on the block-scaled MFMA
(csrc/gemm_mx.hip).  Yardstick: the SAME engine on the CPU reference of the MX ops (tests/ref_ops_mx.py), which quantises with
weights.py:quantize_blocks_mxfp8 and multiplies (A', W') in bf16.  Equal greedy tokens, eviction traces and KV lengths; the smallest
top-2 margin at least 10x the measured absolute logit noise; every forward's logits within 2.5x the CPU reference's OWN re-tiling noise
(its MX GEMMs summed as two K halves in fp32) + 5e-4 (mean, relative to the logit range) and + 5e-3 (max) -- the constants of
tests/test_engine_gpu.py:_compare.  The GPU code never enters the yardstick."""
import pytest
import torch

import helpers as H
from ref_ops_mx import RefOpsMx
from test_stream_group_fp8_gpu import _same_stream, _solo_and_group, _stream_kw

pytestmark = pytest.mark.gpu
Q25 = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8, previous_text="a b c d e f g h i j k l m n o p")


def _gpu_model(cfg, sd, **kw):
    import streaming_vlm_amd as S
    model = S.StreamingQwen2VL(cfg, {k: v.cuda() for k, v in sd.items()}, "cuda", llm_fp4=True, prefill_mx=True, **kw)
    eng = model._svlm_engine
    assert eng.prefill_mx and eng.llm_fp4 and not eng.prefill_fp4
    return model


def _cpu_model(cfg, sd, k_halves=False, max_len=768, max_new_tokens=8, share=None):
    """`share`: the other summation order runs on the first model's weights (one quantisation of the matrices for both)."""
    import streaming_vlm_amd as S
    return S.StreamingQwen2VL(cfg, sd, "cpu", ops=RefOpsMx(k_halves=k_halves), max_len=max_len, max_new_tokens=max_new_tokens, use_graph=False,
                              llm_fp4=True, prefill_mx=True, share=share)


def _rel(a, b):
    d = (a - b).abs()
    sc = float(b.abs().max())
    return float(d.max()) / sc, float(d.mean()) / sc


def _against_the_cpu_reference(cfg, sd, gpu, n_chunks, what, prepare=None, **kw):
    ref_model = _cpu_model(cfg, sd)
    alt_model = _cpu_model(cfg, None, k_halves=True, share=ref_model._svlm_engine)
    for m in (ref_model, alt_model, gpu):
        if prepare:
            prepare(m._svlm_engine)
    _, rtrace, rcounts, ref = H.run_engine_stream(ref_model, n_chunks, keep_logits=True, **kw)
    force = [e["new"][:len(e["logits"])] for e in ref]
    _, _, _, alt = H.run_engine_stream(alt_model, n_chunks, keep_logits=True, force_tokens=force, **kw)
    _, trace, counts, got = H.run_engine_stream(gpu, n_chunks, keep_logits=True, force_tokens=force, **kw)
    assert trace == rtrace, f"{what}: eviction traces differ"
    assert counts == rcounts and len(got) == len(ref)
    fmax = fmean = wmax = wmean = noise = 0.0
    margin = 1e30
    n = 0
    for g, r, a in zip(got, ref, alt):
        assert g["kv_len"] == r["kv_len"] and g["ids"] == r["ids"], what
        assert len(g["logits"]) == len(r["logits"]) == len(a["logits"])
        for u, v, w in zip(g["logits"], r["logits"], a["logits"]):
            f = _rel(w, v)
            fmax, fmean = max(fmax, f[0]), max(fmean, f[1])
            t = torch.topk(v, 2).values
            margin = min(margin, float(t[0] - t[1]))
            n += 1
    for g, r in zip(got, ref):
        for u, v in zip(g["logits"], r["logits"]):
            u = u.cpu()
            mx, mn = _rel(u, v)
            wmax, wmean, noise = max(wmax, mx), max(wmean, mn), max(noise, float((u - v).abs().max()))
            assert mn <= 2.5 * fmean + 5e-4, (what, mn, fmean)
            assert mx <= 2.5 * fmax + 5e-3, (what, mx, fmax)
    own = [e["own"] for e in got]
    print(f"[prefill_mx {what}] {n} forwards; GPU vs CPU MX reference: max rel {wmax:.3e} mean rel {wmean:.3e}, |logit noise| {noise:.3e}, "
          f"smallest top-2 margin {margin:.3e}; reference re-tiling floor max {fmax:.3e} mean {fmean:.3e}")
    assert margin >= 10 * noise, f"{what}: not decisive: margin {margin:.3e} vs noise {noise:.3e}"
    assert own == force, f"{what}: greedy tokens differ\n{own}\n{force}"
    assert gpu._svlm_engine._fp8_scratch is None, "the scratch layer was allocated"
    return trace


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_tiny_streams_equal_the_cpu_mx_reference(family):
    """Graph replay on (the default); sink + window eviction (qwen2), the structural policy (qwen2_5)."""
    from streaming_vlm_amd import config as C
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    gpu = _gpu_model(cfg, sd, max_len=768, max_new_tokens=8)
    assert gpu._svlm_engine.use_graph
    trace = _against_the_cpu_reference(cfg, sd, gpu, 5, f"tiny {family}", **(Q25 if family == "qwen2_5" else {}))
    assert sum(1 for t in trace if t) >= 1, "the stream must evict for this test to mean anything"


def test_dense_prefill_in_48_row_passes():
    from streaming_vlm_amd import config as C
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    gpu = _gpu_model(cfg, sd, max_len=768, max_new_tokens=8)

    def prepare(eng):
        eng.PREFILL_ROWS, eng.VIT_BATCH_SEQS = 48, 2
    passes = []
    eng = gpu._svlm_engine
    inner = eng._prefill

    def spy(c, idx_dev, vis, T, L_before, head=True):
        passes.append((T, L_before))
        return inner(c, idx_dev, vis, T, L_before, head=head)
    eng._prefill = spy
    _against_the_cpu_reference(cfg, sd, gpu, 9, "dense prefill, 48-row passes", prepare=prepare, window=64, dense_prefill_chunks=6)
    assert sum(1 for T, L in passes if L > 0 and T > 1) >= 2 and max(T for T, _ in passes) <= 48, passes


def test_7b_width_stream_runs_the_590_row_shapes_through_the_mx_gemms():
    """Qwen2-VL-7B widths, 2 LLM layers / 1 ViT block, 448 x 448 at 4 frames per second, 2 chunks: M ~ 590 prefills through the quantiser
    and the MX GEMMs (qkv 4608 x 3584, o_proj 3584 x 3584, gate/up SwiGLU 18944 x 3584, down_proj 3584 x 18944), no scratch layer."""
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    cfg = C.qwen2_vl_7b()
    cfg.text.num_layers, cfg.vision.depth = 2, 1
    sd = random_state_dict(cfg, 0, "cpu")
    gpu = _gpu_model(cfg, sd, max_len=4608, max_new_tokens=4)
    o = gpu._svlm_engine.ops
    seen = []
    inner = {n: getattr(o, n) for n in ("quant_mxfp8", "gemm_mx_a8w4", "gemm_mx_a8w4_norm")}

    def spy(name):
        def f(A, *a, **k):
            seen.append((name, int(A.shape[0]), int(A.shape[1])))
            return inner[name](A, *a, **k)
        return f
    for n in inner:
        setattr(o, n, spy(n))
    try:
        _, _, counts, log = H.run_engine_stream(gpu, 2, keep_logits=True, size=448, fps=4.0, window=4096, max_new=4)
    finally:
        for n in inner:
            delattr(o, n)
    assert len(seen) == 2 * 2 * 8 and all(520 <= m <= 640 for _, m, _ in seen), seen
    assert {k for n, _, k in seen if n != "quant_mxfp8"} == {3584, 18944} and sum(1 for n, _, _ in seen if n == "quant_mxfp8") == 16
    assert counts == [4, 4] and all(bool(torch.isfinite(l).all()) for e in log for l in e["logits"])
    assert gpu._svlm_engine._fp8_scratch is None


def test_two_lane_stream_group_equals_the_solo_prefill_mx_streams():
    from streaming_vlm_amd import config as C
    cfg = C.tiny()
    sd = H.decisive_weights(cfg, size=(112, 84))
    model = _gpu_model(cfg, sd, max_len=768, max_new_tokens=8)
    streams = [_stream_kw(cfg, 56, 6, "hello world", "Commentate on this match"),
               _stream_kw(cfg, (112, 84), 4, "the game begins", "What happens now", window=96)]
    solo, grouped = _solo_and_group(cfg, model, streams, 2)
    for i, (g, w) in enumerate(zip(grouped, solo)):
        assert sum(1 for t in w[1]["trace"] if t) >= 1
        _same_stream(i, g, w)
    assert model._svlm_engine._fp8_scratch is None
