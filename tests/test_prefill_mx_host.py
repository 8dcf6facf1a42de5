"""`SvlmEngine(llm_fp4=True, prefill_mx=True)`, host side (no GPU): every prefill pass quantises the A operand of its four GEMMs per
layer to MXFP8 (ops.quant_mxfp8) and multiplies codes by codes (ops.gemm_mx_a8w4 / gemm_mx_a8w4_norm) on the engine's own MXFP4
tensors, never dequantises and never allocates the scratch layer; the accuracy pin against the bf16-activation `llm_fp4` engine on the
same weights; refusals; header / ctypes agreement; the dispatch mirror against the diagnostic library's plan notes; and a torch
emulation of the kernel's tile loop (fragment addressing, A- and W-scale indexing, nibble order, k_begin per split) against the
`blocks` cases of tests/gemm_mx_paths.py, with the faults those cases are there to catch injected one by one."""
import ctypes
import os
import re

import pytest
import torch

import gemm_mx_paths as P
import gemm_ref64 as R
import helpers as H
from ref_ops_fp8 import RefOpsFp8
from ref_ops_mx import RefOpsMx
from ref_ops_wfp4 import RefOpsWfp4
from test_llm_fp4_host import _model

from streaming_vlm_amd import config as C
from streaming_vlm_amd.engine import MX_PREFILL_OPS, SvlmEngine
from streaming_vlm_amd.weights import E2M1_VALUES, random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
Q25 = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8, previous_text="a b c d e f g h i j k l m n o p")
# the four tiny decisive streams: family, what the weights are decisive for, stream kwargs (those of tests/test_engine_gpu.py)
STREAMS = {"qwen2 sink/window": ("qwen2", {}, {}), "qwen2_5 structural": ("qwen2_5", {}, Q25),
           "qwen2_5 video": ("qwen2_5", dict(size=(112, 84)), dict(size=(112, 84), window=96)),
           "qwen2_5 all-text": ("qwen2_5", dict(all_text=True), dict(all_text=True))}


class Recording(RefOpsMx):
    """Counts the calls the prefill makes and keeps the operands of the MX entries."""

    def __init__(self):
        super().__init__()
        self.calls = []
        self._inside = False

    def dequant_fp4(self, W4, w_scale, out):
        self.calls.append(("dequant_fp4", None, None, None))
        return super().dequant_fp4(W4, w_scale, out)

    def gemm(self, A, W, **kw):
        if A.shape[0] > 1 and not self._inside:
            self.calls.append(("gemm", W, None, None))
        return super().gemm(A, W, **kw)

    def gemm_wfp4(self, A, W4, w_scale, **kw):
        self.calls.append(("gemm_wfp4", W4, w_scale, None))
        return super().gemm_wfp4(A, W4, w_scale, **kw)

    def gemm_wfp4_norm(self, A, W4, w_scale, *a, **kw):
        self.calls.append(("gemm_wfp4_norm", W4, w_scale, None))
        return super().gemm_wfp4_norm(A, W4, w_scale, *a, **kw)

    def quant_mxfp8(self, x, q=None, scale=None):
        out = super().quant_mxfp8(x, q, scale)
        self.calls.append(("quant_mxfp8", None, None, (out[0], out[1], tuple(x.shape))))
        return out

    def _mx(self, name, fn, A8, a_scale, W4, w_scale, *a, **kw):
        self.calls.append((name, W4, w_scale, (A8, a_scale, tuple(A8.shape))))
        self._inside = True
        try:
            return fn(A8, a_scale, W4, w_scale, *a, **kw)
        finally:
            self._inside = False

    def gemm_mx_a8w4(self, A8, a_scale, W4, w_scale, **kw):
        return self._mx("gemm_mx_a8w4", super().gemm_mx_a8w4, A8, a_scale, W4, w_scale, **kw)

    def gemm_mx_a8w4_norm(self, A8, a_scale, W4, w_scale, *a, **kw):
        return self._mx("gemm_mx_a8w4_norm", super().gemm_mx_a8w4_norm, A8, a_scale, W4, w_scale, *a, **kw)


def _assert_mx_prefills(ops, eng, n_prefills):
    """Per prefill pass and layer: quantise, qkv; quantise, o_proj + norm; quantise, gate/up; quantise, down_proj (+ norm) -- on the
    engine's own tensors, every GEMM on the codes its quantiser call just wrote."""
    names = [c[0] for c in ops.calls]
    assert not [n for n in names if n == "dequant_fp4" or n.startswith("gemm_wfp4")], set(names)
    layers = eng.w.layers
    mx = [c for c in ops.calls if c[0] in MX_PREFILL_OPS]
    per = 8 * len(layers)
    assert len(mx) == per * n_prefills, (len(mx), per, n_prefills)
    tc = eng.cfg.text
    widths = (tc.hidden_size, eng.qd, tc.hidden_size, tc.intermediate_size)
    for p in range(n_prefills):
        rows = mx[p * per][3][2][0]
        for li, lw in enumerate(layers):
            got = mx[p * per + 8 * li:p * per + 8 * li + 8]
            last = li + 1 == len(layers)
            assert [g[0] for g in got] == ["quant_mxfp8", "gemm_mx_a8w4", "quant_mxfp8", "gemm_mx_a8w4_norm", "quant_mxfp8", "gemm_mx_a8w4",
                                           "quant_mxfp8", "gemm_mx_a8w4" if last else "gemm_mx_a8w4_norm"]
            for j, name in enumerate(("qkv_w", "o_w", "gu_w", "down_w")):
                qz, g = got[2 * j], got[2 * j + 1]
                assert g[1] is lw[name + "4"] and g[2] is lw[name + "_s4"], (li, name)
                assert qz[3][2] == (rows, widths[j]) == g[3][2], (li, name, qz[3][2], g[3][2])
                assert g[3][0] is qz[3][0] and g[3][1] is qz[3][1], "the GEMM reads the codes and scales its quantiser call wrote"
                assert g[3][0].dtype == torch.uint8 and g[3][1].dtype == torch.uint8 and tuple(g[3][1].shape) == (rows, widths[j] // 32)
        # the code and scale buffers are allocated once per pass, not per layer
        first = {w_: mx[p * per + 2 * j][3][0] for j, w_ in enumerate(widths)}
        for li in range(len(layers)):
            for j, w_ in enumerate(widths):
                assert mx[p * per + 8 * li + 2 * j][3][0] is first[w_]
    lm = {id(t) for lw in layers for t in lw.values() if torch.is_tensor(t)}
    assert not [c for c in ops.calls if c[0] == "gemm" and id(c[1]) in lm], "a bf16 GEMM read a language-model matrix"
    assert eng._fp8_scratch is None and eng._fp8_scratch_owner._fp8_scratch is None, "the scratch layer was allocated"
    return mx


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_prefill_issues_four_quantiser_calls_and_four_mx_gemms_per_layer(family):
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    model = _model(cfg, sd, ops, llm_fp4=True, prefill_mx=True)
    eng = model._svlm_engine
    assert eng.prefill_mx and eng.llm_fp4 and not eng.prefill_fp4 and not eng.prefill_fp8
    ops.calls.clear()
    n_chunks = 3
    H.run_engine_stream(model, n_chunks, **(Q25 if family == "qwen2_5" else {}))
    _assert_mx_prefills(ops, eng, n_chunks)
    # decode is the llm_fp4 engine's: the same stream on RefOpsMx without the flag goes through the scratch layer and no MX entry
    ops2 = Recording()
    scratch = _model(cfg, sd, ops2, llm_fp4=True)
    ops2.calls.clear()
    H.run_engine_stream(scratch, 1)
    assert not [c for c in ops2.calls if c[0] in MX_PREFILL_OPS] and scratch._svlm_engine._fp8_scratch is not None


def test_dense_prefill_runs_several_mx_passes_with_rows_in_front():
    """PREFILL_ROWS lowered to 48 and dense_prefill_chunks=6: passes with L_before > 0, every one through the MX GEMMs whatever its
    row count; tokens, traces and KV lengths equal the bf16-activation llm_fp4 engine's."""
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    model = _model(cfg, sd, ops, llm_fp4=True, prefill_mx=True)
    eng = model._svlm_engine
    eng.PREFILL_ROWS, eng.VIT_BATCH_SEQS = 48, 2
    before = []
    inner = eng._prefill

    def spy(c, idx_dev, vis, T, L_before, head=True):
        before.append((T, L_before))
        return inner(c, idx_dev, vis, T, L_before, head=head)
    eng._prefill = spy
    ops.calls.clear()
    kw = dict(window=64, dense_prefill_chunks=6)
    got = H.run_engine_stream(model, 9, keep_logits=True, **kw)
    assert sum(1 for T, L in before if L > 0 and T > 1) >= 2 and max(T for T, _ in before) <= 48, before
    _assert_mx_prefills(ops, eng, len(before))
    base = _model(cfg, sd, RefOpsWfp4(), llm_fp4=True)
    base._svlm_engine.PREFILL_ROWS, base._svlm_engine.VIT_BATCH_SEQS = 48, 2
    want = H.run_engine_stream(base, 9, keep_logits=True, **kw)
    assert got[1] == want[1] and [e["ids"] for e in got[3]] == [e["ids"] for e in want[3]]
    assert [e["kv_len"] for e in got[3]] == [e["kv_len"] for e in want[3]]


def _stream_logits(model, n_chunks, force=None, **kw):
    extra = dict(force_tokens=force) if force is not None else {}
    _, trace, _, log = H.run_engine_stream(model, n_chunks, keep_logits=True, **extra, **kw)
    return trace, log


def _rel(a, b):
    d = (a - b).abs()
    sc = float(b.abs().max())
    return float(d.max()) / sc, float(d.mean()) / sc, float(d.max())


def _margin(logits):
    t = torch.topk(logits, 2).values
    return float(t[0] - t[1])


@pytest.mark.parametrize("name", list(STREAMS))
def test_accuracy_pin_against_the_bf16_activation_fp4_engine(name):
    """Same weights, 7 chunks: the prefill_mx engine on RefOpsMx against the llm_fp4 engine on RefOpsWfp4.  Equal greedy tokens, eviction
    traces and KV lengths; the smallest raw top-2 margin of the deciding logits is at least 10x the largest absolute logit difference
    between the two engines (the decisiveness rule of tests/test_engine_gpu.py:_compare).  Prints the distances DESIGN section 7 quotes,
    and the MX reference's own re-tiling noise (the same GEMMs summed as two K halves in fp32)."""
    family, decisive_for, kw = STREAMS[name]
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg, **decisive_for)
    base = _stream_logits(_model(cfg, sd, RefOpsWfp4(), llm_fp4=True), 7, **kw)
    force = [e["new"][:len(e["logits"])] for e in base[1]]          # one token per forward (the appended end-of-turn token aside)
    mx = _stream_logits(_model(cfg, sd, RefOpsMx(), llm_fp4=True, prefill_mx=True), 7, **kw)
    assert mx[0] == base[0], "eviction traces differ"
    assert [e["ids"] for e in mx[1]] == [e["ids"] for e in base[1]] and [e["new"] for e in mx[1]] == [e["new"] for e in base[1]], "greedy tokens differ"
    assert [e["kv_len"] for e in mx[1]] == [e["kv_len"] for e in base[1]]
    alt = _stream_logits(_model(cfg, sd, RefOpsMx(k_halves=True), llm_fp4=True, prefill_mx=True), 7, force=force, **kw)
    wmax = wmean = noise = fmax = fmean = 0.0
    margin = 1e30
    n = 0
    for a, b, c in zip(mx[1], base[1], alt[1]):
        assert len(a["logits"]) == len(b["logits"]) == len(c["logits"]) > 0
        for u, v, w in zip(a["logits"], b["logits"], c["logits"]):
            r = _rel(u, v)
            wmax, wmean, noise = max(wmax, r[0]), max(wmean, r[1]), max(noise, r[2])
            f = _rel(w, u)
            fmax, fmean = max(fmax, f[0]), max(fmean, f[1])
            margin = min(margin, _margin(v))
            n += 1
    print(f"[prefill_mx pin, {name}] {n} forwards: max rel {wmax:.3e} mean rel {wmean:.3e}, largest |logit difference| {noise:.3e}, "
          f"smallest top-2 margin {margin:.3e}; MX reference re-tiling noise max {fmax:.3e} mean {fmean:.3e}")
    assert margin >= 10 * noise, f"not decisive: smallest top-2 margin {margin:.3e} vs logit difference {noise:.3e}"


def test_prefill_mx_refusals():
    assert MX_PREFILL_OPS == ("quant_mxfp8", "gemm_mx_a8w4", "gemm_mx_a8w4_norm")
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    with pytest.raises(ValueError, match="prefill_mx=True needs llm_fp4=True"):
        _model(cfg, sd, RefOpsMx(), prefill_mx=True)
    with pytest.raises(ValueError, match="needs llm_fp4=True"):
        _model(cfg, sd, RefOpsMx(), llm_fp8=True, prefill_mx=True)
    with pytest.raises(ValueError):
        _model(cfg, sd, RefOpsMx(), llm_fp8=True, prefill_fp8=True, prefill_mx=True)
    with pytest.raises(ValueError, match="prefill_mx=True cannot be combined with prefill_fp4=True"):
        _model(cfg, sd, RefOpsMx(), llm_fp4=True, prefill_fp4=True, prefill_mx=True)
    with pytest.raises(ValueError, match="decode_tail"):
        _model(cfg, sd, RefOpsMx(), llm_fp4=True, prefill_mx=True, decode_tail=True)
    with pytest.raises(ValueError, match="MX quantiser and GEMMs.*quant_mxfp8.*gemm_mx_a8w4"):
        _model(cfg, sd, RefOpsWfp4(), llm_fp4=True, prefill_mx=True)
    with pytest.raises(ValueError, match="fp4 entry points"):
        _model(cfg, sd, RefOpsFp8(), llm_fp4=True, prefill_mx=True)          # an fp8-only backend
    odd = C.tiny()
    odd.text.intermediate_size = 576          # a multiple of 64 (prefill_fp4 takes it), not of 128
    with pytest.raises(ValueError, match="multiple of 128.*intermediate is 576"):
        _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsMx(), llm_fp4=True, prefill_mx=True)
    assert _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsMx(), llm_fp4=True, prefill_fp4=True)._svlm_engine.prefill_mx is False
    # engines that share weights must agree on the flag
    base = _model(cfg, sd, RefOpsMx(), llm_fp4=True, prefill_mx=True)._svlm_engine
    with pytest.raises(ValueError, match="prefill_mx"):
        SvlmEngine(cfg, None, "cpu", llm_fp4=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    plain = _model(cfg, sd, RefOpsMx(), llm_fp4=True)._svlm_engine
    with pytest.raises(ValueError, match="prefill_mx"):
        SvlmEngine(cfg, None, "cpu", llm_fp4=True, prefill_mx=True, share=plain, max_len=1024, max_new_tokens=8, use_graph=False)
    lane = SvlmEngine(cfg, None, "cpu", llm_fp4=True, prefill_mx=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    assert lane.prefill_mx and lane.w is base.w and lane.ops is base.ops


def test_lanes_that_share_the_weights_prefill_through_the_mx_gemms_and_give_the_solo_tokens():
    """What a stream group's lanes are on the host side: engines built with share= on a prefill_mx engine (StreamGroup passes the flag
    on).  Two such lanes run the stream one after the other, through the same `_prefill`: each gives the solo stream's tokens, traces
    and KV lengths, and neither dequantises.  (The lane-batched decode step itself needs the GPU: tests/test_prefill_mx_gpu.py.)"""
    import inspect
    from types import MethodType
    import streaming_vlm_amd as S
    from streaming_vlm_amd import stream_group as SG
    assert "prefill_mx=" in inspect.getsource(SG.StreamGroup.__init__), "a group hands the flag to its lanes"
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    solo = _model(cfg, sd, ops, llm_fp4=True, prefill_mx=True)
    want = H.run_engine_stream(solo, 4)
    lanes = []
    for _ in range(2):
        m = S.StreamingQwen2VL.__new__(S.StreamingQwen2VL)
        m.config, m.device = cfg, torch.device("cpu")
        m._svlm_engine = SvlmEngine(cfg, None, "cpu", ops=ops, llm_fp4=True, prefill_mx=True, share=solo._svlm_engine, max_len=1024,
                                    max_new_tokens=8, use_graph=False)
        m.generate = MethodType(S.streaming_generate, m)
        lanes.append(m)
    ops.calls.clear()
    for m in lanes:
        got = H.run_engine_stream(m, 4)
        assert got[1] == want[1] and got[2] == want[2] and [e["ids"] for e in got[3]] == [e["ids"] for e in want[3]]
    assert not [c for c in ops.calls if c[0] == "dequant_fp4"] and solo._svlm_engine._fp8_scratch is None
    assert sum(1 for c in ops.calls if c[0] == "quant_mxfp8") == 2 * 4 * 4 * len(solo._svlm_engine.w.layers)


def test_header_declares_and_the_ctypes_table_binds_the_three_entries():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))
    args = lambda n: [a.strip() for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()]
    for n in ("svlm_quant_mxfp8", "svlm_gemm_mx_a8w4", "svlm_gemm_mx_a8w4_norm"):
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES and getattr(lib, n)
        assert len(args(n)) == len(_lib.SIGNATURES[n][1]), n
        assert callable(getattr(HipOps, n[len("svlm_"):]))
        for a, t in zip(args(n), _lib.SIGNATURES[n][1]):
            want = ctypes.c_void_p if "*" in a else {"int": ctypes.c_int, "long long": ctypes.c_longlong, "float": ctypes.c_float}[a.rsplit(" ", 1)[0]]
            assert t is want, (n, a, t)
    # the wfp4 twins' argument lists with A -> (A8, a_scale)
    for n, twin in (("svlm_gemm_mx_a8w4", "svlm_gemm_wfp4"), ("svlm_gemm_mx_a8w4_norm", "svlm_gemm_wfp4_norm")):
        t = args(twin)
        assert args(n) == ["const void* A8", t[1], "const void* a_scale"] + t[2:], (n, args(n))
    assert args("svlm_quant_mxfp8") == [a.replace("float* scale", "void* scale") for a in args("svlm_quant_rows_fp8")]
    assert _lib.load().svlm_abi_version() == 1
    full = open(os.path.join(ROOT, "include", "svlm.h")).read()
    assert "replaces: nothing, the reference has bf16 activations" in full


def _host_plan(lib, M, N, K, act, norm, env):
    with H.forced_switches(env):          # goes to the C environment the diagnostic library reads
        v = (ctypes.c_int * 10)()
        lib.svlm_diag_last_gemm_plan(v, 10)
        seq = v[0]
        fake = ctypes.c_void_p(4096)
        a = [fake, K, fake, fake, K // 2, fake, None, None, 0, fake, N, M, N, K, act, fake, P.WS_BYTES]
        if norm:
            lib.svlm_gemm_mx_a8w4_norm(*a, fake, None, 1e-6, fake, N, None)
        else:
            lib.svlm_gemm_mx_a8w4(*a, None)
        lib.svlm_diag_last_gemm_plan(v, 10)
        assert v[0] == seq + 1, f"the call was rejected before it planned: {lib.svlm_last_error()}"
        return dict(fp8=v[1], bm=v[2], waves=v[3], stages=v[4], dma=v[5], splits=v[6], kps=v[7], table=v[8])


def test_mx_mirror_matches_the_library_plan():
    """The diagnostic library notes the plan of a svlm_gemm_mx_a8w4 call before it touches the device (the technique of
    tests/test_prefill_fp4_host.py::test_wfp4_mirror_matches_the_library_plan), so tests/gemm_mx_paths.py:plan_mx is pinned to
    gemm_mx_impl without a GPU: every case of the GPU table and a grid of shapes around the tile and split boundaries."""
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gemm_mx_gpu.py asserts the reported plan of real launches instead")
    from test_gemm_ref64 import _diag_lib
    lib = _diag_lib()
    n = 0
    for c in P.CASES:
        want = P.plan_mx(c["M"], c["N"], c["K"], act=c["act"], norm=c["norm"] is not None, env=c["force"])
        got = _host_plan(lib, c["M"], c["N"], c["K"], c["act"], c["norm"] is not None, c["force"])
        assert got == {k: want[k] for k in got}, (c["id"], got, want)
        n += 1
    shapes = [(4608, 3584), (3584, 3584), (18944, 3584), (3584, 18944), (2048, 1536), (1536, 1536), (8960, 1536), (1536, 8960),
              (264, 4096), (1024, 256), (256, 512), (132, 896), (128, 1024), (37888, 3584)]
    for N, K in shapes:
        for M in (1, 63, 64, 65, 128, 129, 255, 256, 257, 290, 511, 512, 513, 590, 1023, 1024, 1025, 2048, 4096):
            for act in ((0, 4) if N % 8 == 0 else (0,)):
                for norm in ((False, True) if act == 0 and N % 8 == 0 else (False,)):
                    want = P.plan_mx(M, N, K, act=act, norm=norm)
                    got = _host_plan(lib, M, N, K, act, norm, None)
                    assert got == {k: want[k] for k in got}, (M, N, K, act, norm, got, want)
                    assert want["kps"] % 128 == 0 and (want["splits"] - 1) * want["kps"] < K
                    n += 1
    assert n > 500 and got["fp8"] == 4
    # the chunk-prefill shapes split K to fill the 256 CUs, the 4096-row passes do not
    for N, K in ((4608, 3584), (3584, 18944), (2048, 1536), (1536, 8960)):
        assert P.plan_mx(290, N, K)["splits"] > 1 and P.plan_mx(590, N, K)["splits"] > 1, (N, K)
        assert P.plan_mx(4096, N, K) == dict(P.plan_mx(4096, N, K), splits=1, bm=128, kps=K)
    # the two switches, and what they refuse
    for env in ({"SVLM_GEMM_MX_BM": "128"}, {"SVLM_GEMM_MX_BM": "64", "SVLM_GEMM_MX_SPLITS": "5"}, {"SVLM_GEMM_MX_SPLITS": "1"},
                {"SVLM_GEMM_MX_SPLITS": "400"}, {"SVLM_GEMM_MX_BM": "96"}):
        want = P.plan_mx(290, 3584, 18944, env=env)
        got = _host_plan(lib, 290, 3584, 18944, 0, False, env)
        assert got == {k: want[k] for k in got}, (env, got, want)
    assert P.plan_mx(290, 3584, 18944, env={"SVLM_GEMM_MX_SPLITS": "5"})["splits"] == 5 != P.plan_mx(290, 3584, 18944)["splits"]


# ------------------------------------------------------------------------------------------------ torch emulation of the tile loop
FAULTS = ("a_next_block", "a_next_row", "a_prev_kstep", "a_no_k_begin", "w_next_block", "w_next_row", "w_prev_kstep", "w_no_k_begin",
          "swapped_nibbles", "a_consecutive_chunks")
_LUT = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32)


def emulate(A8, sa, W4, s, plan, fault=None):
    """What gemm_mx_kernel computes for C = A' . W'^T, addressed as the kernel addresses it and multiplied as the scaled MFMA multiplies
    it (operand layout: csrc/gemm_mx.hip).  Per K-split (k_begin = split * kps) and K-step kt of 128 the instruction sees 128 k slots in
    four blocks of 32; block j of a row is scaled by the byte lane group j holds: row * (K / 32) + k_begin / 32 + 4 kt + j, either
    operand.  W (e2m1): lane group fq fills slots 32 fq .. 32 fq + 31 from the 16 bytes at row * ldw + k_begin / 2 + 64 kt + 16 fq
    (element 2i in the low nibble of byte i).  A (e4m3): lane group fq fills slots 16 fq .. + 15 from the 16-B chunk fq and slots
    64 + 16 fq .. + 15 from chunk 4 + fq of the 128 bytes at row * lda + k_begin + 128 kt.  Products in fp32 per split, the splits summed
    in fp32, one rounding to bf16.  `fault`: one of FAULTS; `a_consecutive_chunks` is the lane that fetches "its own" block (chunks 2 fq
    and 2 fq + 1), which the hardware multiplies with the wrong weights."""
    M, K = A8.shape
    N = W4.shape[0]
    nb = K // 32
    rawa, raw4, rsa, rsw = A8.reshape(-1), W4.reshape(-1), sa.reshape(-1), s.reshape(-1)
    mrows, nrows = torch.arange(M), torch.arange(N)
    lut8 = torch.arange(256, dtype=torch.uint8).view(FP8).float()
    out = torch.zeros((M, N), dtype=torch.float32)

    def scale(raw, rows, n_rows, k_begin, kt, j, who):
        idx = ((0 if fault == who + "_no_k_begin" else k_begin // 32) + 4 * kt + j + (1 if fault == who + "_next_block" else 0)
               - (4 if fault == who + "_prev_kstep" else 0)) % nb
        r = (rows + 1) % n_rows if fault == who + "_next_row" else rows
        return torch.pow(2.0, raw[r * nb + idx].float() - 127)
    for split in range(plan["splits"]):
        k_begin = split * plan["kps"]
        k_end = min(K, k_begin + plan["kps"])
        part = torch.zeros_like(out)
        for kt in range((k_end - k_begin) // 128):
            a_hw, w_hw = torch.zeros((M, 128)), torch.zeros((N, 128))
            for fq in range(4):
                chunks = (2 * fq, 2 * fq + 1) if fault == "a_consecutive_chunks" else (fq, 4 + fq)
                for h, c in enumerate(chunks):
                    ab = rawa[(mrows * K + k_begin + kt * 128 + 16 * c)[:, None] + torch.arange(16)[None, :]]                 # [M, 16]
                    a_hw[:, 64 * h + 16 * fq:64 * h + 16 * fq + 16] = lut8[ab.long()]
                wb = raw4[(nrows * (K // 2) + k_begin // 2 + kt * 64 + fq * 16)[:, None] + torch.arange(16)[None, :]]      # [N, 16]
                lo, hi = _LUT[(wb & 0xF).long()], _LUT[(wb >> 4).long()]
                w_hw[:, 32 * fq:32 * fq + 32] = torch.stack([hi, lo] if fault == "swapped_nibbles" else [lo, hi], dim=-1).view(N, 32)
            for j in range(4):
                a_hw[:, 32 * j:32 * j + 32] *= scale(rsa, mrows, M, k_begin, kt, j, "a")[:, None]
                w_hw[:, 32 * j:32 * j + 32] *= scale(rsw, nrows, N, k_begin, kt, j, "w")[:, None]
            part += a_hw @ w_hw.t()
        out += part
    return out.to(BF16)


def test_tile_loop_emulation_is_exact_and_every_injected_fault_breaks_the_bound():
    """The emulation is exact on every `blocks` case (one product per output, every block of either operand its own scale byte); each
    of the ten faults exceeds the fp8-MFMA bound on at least one of them -- the ones that need a K-split only there."""
    assert len(P.SMALL_BLOCKS) >= 10
    plans = [P.plan_mx(c["M"], c["N"], c["K"], env=c["force"]) for c in P.SMALL_BLOCKS]
    assert any(p["splits"] > 1 for p in plans) and any(p["splits"] == 1 for p in plans)
    caught = {f: [] for f in FAULTS}
    for c, plan in zip(P.SMALL_BLOCKS, plans):
        o = P.operands("blocks", c["M"], c["N"], c["K"])
        ref, bound, _, _ = R.reference(o["Ap"], o["Wp"], c=R.fadds(dict(plan, fp8=1), c["K"]))
        got = emulate(o["A8"], o["sa"], o["W4"], o["s"], plan)
        ratio, _ = R.ratios(got, ref, bound)
        assert float(ratio.max()) <= 1.0 and bool((got.double() == ref).all()), c["id"]
        for f in FAULTS:
            if f.endswith("no_k_begin") and plan["splits"] == 1:
                continue
            ratio, _ = R.ratios(emulate(o["A8"], o["sa"], o["W4"], o["s"], plan, fault=f), ref, bound)
            if float(ratio.max()) > 1.0:
                caught[f].append(c["id"])
    print({f: len(v) for f, v in caught.items()})
    assert all(caught[f] for f in FAULTS), {f: len(v) for f, v in caught.items()}
