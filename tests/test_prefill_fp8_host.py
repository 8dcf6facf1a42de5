"""`SvlmEngine(llm_fp8=True, prefill_fp8=True)`, host side (no GPU): the prefill issues its four GEMMs per layer on the e4m3 codes and
their row scales (ops.gemm_wfp8 / gemm_wfp8_norm), never dequantises and never allocates the scratch layer; on the CPU reference of those
ops it is the bf16 engine on W' = fp8_reference_state_dict(W), bit for bit."""
import ctypes
import os
import re

import pytest
import torch

import helpers as H
from ref_ops import RefOps
from ref_ops_fp8 import RefOpsFp8
from ref_ops_wfp8 import RefOpsWfp8
from test_llm_fp8_host import _model, untied

from streaming_vlm_amd import config as C
from streaming_vlm_amd.stream_group import FP8_GROUP_OPS, StreamGroup
from streaming_vlm_amd.weights import fp8_reference_state_dict, random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_prefill_fp8_engine_is_the_bf16_engine_on_the_dequantised_weights(family):
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    sdp = fp8_reference_state_dict(sd, cfg)
    kw = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8) if family == "qwen2_5" else {}
    outs = []
    for model in (_model(cfg, sd, RefOpsWfp8(), llm_fp8=True, prefill_fp8=True), _model(untied(cfg), sdp, RefOps())):
        res, trace, counts, log = H.run_engine_stream(model, 4, keep_logits=True, **kw)
        outs.append((trace, [e["ids"] for e in log], [e["kv_len"] for e in log], [torch.stack(e["logits"]) for e in log]))
    assert outs[0][:3] == outs[1][:3]
    for a, b in zip(outs[0][3], outs[1][3]):
        assert torch.equal(a, b)


class Recording(RefOpsWfp8):
    """Counts the calls the prefill makes and keeps the weight operands of the weight-fp8 GEMMs."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def dequant_fp8(self, W8, w_scale, out):
        self.calls.append(("dequant_fp8", None, None))
        return super().dequant_fp8(W8, w_scale, out)

    def gemm(self, A, W, **kw):
        if A.shape[0] > 1 and not getattr(self, "_inside", False):
            self.calls.append(("gemm", W, None))
        return super().gemm(A, W, **kw)

    def gemm_wfp8(self, A, W8, w_scale, **kw):
        self.calls.append(("gemm_wfp8", W8, w_scale))
        self._inside = True
        try:
            return super().gemm_wfp8(A, W8, w_scale, **kw)
        finally:
            self._inside = False

    def gemm_wfp8_norm(self, A, W8, w_scale, *a, **kw):
        self.calls.append(("gemm_wfp8_norm", W8, w_scale))
        self._inside = True
        try:
            return super().gemm_wfp8_norm(A, W8, w_scale, *a, **kw)
        finally:
            self._inside = False


def test_prefill_issues_four_weight_fp8_gemms_per_layer_and_never_dequantises():
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    model = _model(cfg, sd, ops, llm_fp8=True, prefill_fp8=True)
    eng = model._svlm_engine
    assert eng.prefill_fp8 and eng.llm_fp8
    ops.calls.clear()                     # (the vision tower's GEMMs of the construction, if any)
    n_chunks = 3
    H.run_engine_stream(model, n_chunks)
    names = [c[0] for c in ops.calls]
    assert names.count("dequant_fp8") == 0
    layers = eng.w.layers
    wf = [c for c in ops.calls if c[0].startswith("gemm_wfp8")]
    assert len(wf) == 4 * len(layers) * n_chunks
    per_prefill = 4 * len(layers)
    for p in range(n_chunks):
        for li, lw in enumerate(layers):
            got = wf[p * per_prefill + 4 * li:p * per_prefill + 4 * li + 4]
            last = li + 1 == len(layers)
            assert [g[0] for g in got] == ["gemm_wfp8", "gemm_wfp8_norm", "gemm_wfp8", "gemm_wfp8" if last else "gemm_wfp8_norm"]
            for g, name in zip(got, ("qkv_w", "o_w", "gu_w", "down_w")):
                assert g[1] is lw[name + "8"] and g[2] is lw[name + "_s"], (li, name)
                assert g[1].dtype == torch.float8_e4m3fn and g[2].dtype == torch.float32
    # the bf16 GEMMs that remain are the vision tower's and the merger's: none reads a language-model matrix
    lm = {id(t) for lw in layers for t in lw.values() if torch.is_tensor(t)}
    assert not [c for c in ops.calls if c[0] == "gemm" and id(c[1]) in lm]
    assert eng._fp8_scratch is None and eng._fp8_scratch_owner._fp8_scratch is None
    # ... while the scratch engine of the same weights does dequantise, four matrices per layer and prefill
    ops2 = Recording()
    scratch = _model(cfg, sd, ops2, llm_fp8=True)
    ops2.calls.clear()
    H.run_engine_stream(scratch, 1)
    assert [c[0] for c in ops2.calls].count("dequant_fp8") == 4 * len(layers) and scratch._svlm_engine._fp8_scratch is not None
    assert not [c for c in ops2.calls if c[0].startswith("gemm_wfp8")]


def test_prefill_fp8_refusals():
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    with pytest.raises(ValueError, match="needs llm_fp8=True"):
        _model(cfg, sd, RefOpsWfp8(), prefill_fp8=True)
    with pytest.raises(ValueError, match="weight-fp8 GEMMs.*gemm_wfp8"):
        _model(cfg, sd, RefOpsFp8(), llm_fp8=True, prefill_fp8=True)
    odd = C.tiny()
    odd.text.intermediate_size = 544          # a multiple of 16 (llm_fp8 takes it), not of 64
    with pytest.raises(ValueError, match="multiple of 64.*intermediate is 544"):
        _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsWfp8(), llm_fp8=True, prefill_fp8=True)
    assert _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsWfp8(), llm_fp8=True)._svlm_engine.prefill_fp8 is False
    # engines that share weights must agree on the flag
    base = _model(cfg, sd, RefOpsWfp8(), llm_fp8=True, prefill_fp8=True)._svlm_engine
    from streaming_vlm_amd.engine import SvlmEngine
    with pytest.raises(ValueError, match="prefill_fp8"):
        SvlmEngine(cfg, None, "cpu", llm_fp8=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    lane = SvlmEngine(cfg, None, "cpu", llm_fp8=True, prefill_fp8=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    assert lane.prefill_fp8 and lane.w is base.w


class GroupOps(RefOpsWfp8):
    """Enough of the lane-batched surface for a group to be CONSTRUCTED on the CPU (nothing here runs a step)."""
    LANE_WORDS = 9

    def decb_sampling_ws(self, V, B, device):
        return torch.zeros(1, dtype=torch.float32, device=device)


for _n in FP8_GROUP_OPS:
    setattr(GroupOps, _n, lambda self, *a, **k: None)


def test_a_group_on_a_prefill_fp8_engine_has_prefill_fp8_lanes():
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    for flag in (True, False):
        eng = _model(cfg, sd, GroupOps(), llm_fp8=True, prefill_fp8=flag)._svlm_engine
        grp = StreamGroup(eng, 3)
        assert len(grp.lanes) == 3 and all(ln.prefill_fp8 is flag and ln.llm_fp8 for ln in grp.lanes)
        assert all(ln.w is eng.w for ln in grp.lanes)


def test_header_declares_and_the_ctypes_table_binds_both_entries():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from streaming_vlm_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))
    twins = {"svlm_gemm_wfp8": "svlm_gemm_bf16", "svlm_gemm_wfp8_norm": "svlm_gemm_bf16_norm"}
    for n, twin in twins.items():
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES and getattr(lib, n)
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[n][1]), n
        assert n_args == len(_lib.SIGNATURES[twin][1]) + 1, "the bf16 twin's arguments with W -> W8, ldw, w_scale"
    assert _lib.load().svlm_abi_version() == 1


def test_wfp8_mirror_matches_the_library_plan():
    """The diagnostic library notes the plan of a svlm_gemm_wfp8 call before it touches the device (as tests/test_gemm_ref64.py uses for
    the bf16 mirror), so tests/gemm_wfp8_paths.py:plan_wfp8 is pinned to gemm_wfp8_impl without a GPU: every case of the GPU test and a
    grid of shapes around the table buckets and the large-M rule."""
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gemm_wfp8_gpu.py asserts the reported plan of real launches instead")
    import gemm_wfp8_paths as P
    from test_gemm_ref64 import _diag_lib
    lib = _diag_lib()
    fake = ctypes.c_void_p(4096)

    def host_plan(M, N, K, act, norm, env):
        with H.forced_switches(env):          # goes to the C environment the diagnostic library reads
            v = (ctypes.c_int * 10)()
            lib.svlm_diag_last_gemm_plan(v, 10)
            seq = v[0]
            a = [fake, K, fake, K, fake, None, None, 0, fake, N, M, N, K, act, fake, P.WS_BYTES]
            if norm:
                lib.svlm_gemm_wfp8_norm(*a, fake, None, 1e-6, fake, N, None)
            else:
                lib.svlm_gemm_wfp8(*a, None)
            lib.svlm_diag_last_gemm_plan(v, 10)
            assert v[0] == seq + 1, f"the call was rejected before it planned: {lib.svlm_last_error()}"
            return dict(fp8=v[1], bm=v[2], waves=v[3], stages=v[4], dma=v[5], splits=v[6], kps=v[7], table=v[8])

    n = 0
    for c in P.CASES:
        want = P.plan_wfp8(c["M"], c["N"], c["K"], act=c["act"], norm=c["norm"] is not None, env=c["force"])
        got = host_plan(c["M"], c["N"], c["K"], c["act"], c["norm"] is not None, c["force"])
        assert got == {k: want[k] for k in got}, (c["id"], got, want)
        n += 1
    shapes = [(N, K) for (_, N, K, _, _) in P.TUNED] + [(2048, 1536), (1536, 1536), (8960, 1536), (260, 4096), (1024, 256)]
    for N, K in shapes:
        for M in (1, 64, 65, 191, 192, 193, 256, 275, 290, 384, 385, 448, 449, 512, 590, 704, 705, 2047, 2048, 2305, 4096):
            for act in ((0, 4) if N % 8 == 0 else (0,)):
                want = P.plan_wfp8(M, N, K, act=act)
                got = host_plan(M, N, K, act, False, None)
                assert got == {k: want[k] for k in got}, (M, N, K, act, got, want)
                n += 1
    assert n > 300 and got["fp8"] == 2


def test_passes_above_the_row_threshold_go_through_the_scratch_layer():
    """`PREFILL_FP8_MAX_ROWS`: a pass of more rows dequantises and runs the bf16 GEMMs (the dense prefill's 4096-row passes); same model,
    same bits.  The threshold is lowered on one engine so that the tiny stream's prefills (tens of rows) cross it."""
    from streaming_vlm_amd.engine import SvlmEngine
    assert SvlmEngine.PREFILL_FP8_MAX_ROWS == 1024 < SvlmEngine.PREFILL_ROWS
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    model = _model(cfg, sd, ops, llm_fp8=True, prefill_fp8=True)
    model._svlm_engine.PREFILL_FP8_MAX_ROWS = 8
    ops.calls.clear()
    got = H.run_engine_stream(model, 2, keep_logits=True)
    names = [c[0] for c in ops.calls]
    assert names.count("dequant_fp8") == 4 * len(model._svlm_engine.w.layers) * 2 and not [n for n in names if n.startswith("gemm_wfp8")]
    assert model._svlm_engine._fp8_scratch is not None
    want = H.run_engine_stream(_model(cfg, sd, RefOpsWfp8(), llm_fp8=True, prefill_fp8=True), 2, keep_logits=True)
    assert got[1] == want[1] and [e["ids"] for e in got[3]] == [e["ids"] for e in want[3]]
    for a, b in zip(got[3], want[3]):
        assert torch.equal(torch.stack(a["logits"]), torch.stack(b["logits"]))
