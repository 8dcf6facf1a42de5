"""`SvlmEngine(llm_fp4=True, prefill_fp4=True)`, host side (no GPU): the prefill issues its four GEMMs per layer on the e2m1 codes and
their block scales (ops.gemm_wfp4 / gemm_wfp4_norm), never dequantises and never allocates the scratch layer; on the CPU reference of
those ops it is the bf16 engine on W' = fp4_reference_state_dict(W), bit for bit.  Also: the dispatch mirror against the diagnostic
library's plan notes, and a torch emulation of the kernel's tile loop (fragment addressing, scale indexing, nibble order) against the
`blocks` cases of tests/gemm_wfp4_paths.py, with the faults those cases are there to catch injected one by one."""
import ctypes
import os
import re

import pytest
import torch

import gemm_ref64 as R
import gemm_wfp4_paths as P
import helpers as H
from ref_ops import RefOps
from ref_ops_fp4 import RefOpsFp4
from ref_ops_wfp4 import RefOpsWfp4
from test_llm_fp4_host import _model, untied

from streaming_vlm_amd import config as C
from streaming_vlm_amd.engine import FP4_LLM_OPS, FP4_PREFILL_OPS, SvlmEngine
from streaming_vlm_amd.stream_group import StreamGroup
from streaming_vlm_amd.weights import E2M1_VALUES, fp4_reference_state_dict, random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


@pytest.mark.parametrize("family", ["qwen2", "qwen2_5"])
def test_prefill_fp4_engine_is_the_bf16_engine_on_the_dequantised_weights(family):
    cfg = C.tiny_2_5() if family == "qwen2_5" else C.tiny()
    sd = H.decisive_weights(cfg)
    sdp = fp4_reference_state_dict(sd, cfg)
    kw = dict(policy="structural", text_round=2, window_size=3, text_sink=4, text_sliding_window=8) if family == "qwen2_5" else {}
    outs = []
    for model in (_model(cfg, sd, RefOpsWfp4(), llm_fp4=True, prefill_fp4=True), _model(untied(cfg), sdp, RefOps())):
        res, trace, counts, log = H.run_engine_stream(model, 4, keep_logits=True, **kw)
        outs.append((trace, [e["ids"] for e in log], [e["kv_len"] for e in log], [torch.stack(e["logits"]) for e in log]))
    assert outs[0][:3] == outs[1][:3]
    for a, b in zip(outs[0][3], outs[1][3]):
        assert torch.equal(a, b)


class Recording(RefOpsWfp4):
    """Counts the calls the prefill makes and keeps the weight operands of the weight-fp4 GEMMs."""

    def __init__(self):
        super().__init__()
        self.calls = []

    def dequant_fp4(self, W4, w_scale, out):
        self.calls.append(("dequant_fp4", None, None))
        return super().dequant_fp4(W4, w_scale, out)

    def gemm(self, A, W, **kw):
        if A.shape[0] > 1 and not getattr(self, "_inside", False):
            self.calls.append(("gemm", W, None))
        return super().gemm(A, W, **kw)

    def gemm_wfp4(self, A, W4, w_scale, **kw):
        self.calls.append(("gemm_wfp4", W4, w_scale))
        self._inside = True
        try:
            return super().gemm_wfp4(A, W4, w_scale, **kw)
        finally:
            self._inside = False

    def gemm_wfp4_norm(self, A, W4, w_scale, *a, **kw):
        self.calls.append(("gemm_wfp4_norm", W4, w_scale))
        self._inside = True
        try:
            return super().gemm_wfp4_norm(A, W4, w_scale, *a, **kw)
        finally:
            self._inside = False


def test_prefill_issues_four_weight_fp4_gemms_per_layer_and_never_dequantises():
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    model = _model(cfg, sd, ops, llm_fp4=True, prefill_fp4=True)
    eng = model._svlm_engine
    assert eng.prefill_fp4 and eng.llm_fp4 and not eng.prefill_fp8
    ops.calls.clear()                     # (the vision tower's GEMMs of the construction, if any)
    n_chunks = 3
    H.run_engine_stream(model, n_chunks)
    names = [c[0] for c in ops.calls]
    assert names.count("dequant_fp4") == 0
    layers = eng.w.layers
    wf = [c for c in ops.calls if c[0].startswith("gemm_wfp4")]
    assert len(wf) == 4 * len(layers) * n_chunks
    per_prefill = 4 * len(layers)
    for p in range(n_chunks):
        for li, lw in enumerate(layers):
            got = wf[p * per_prefill + 4 * li:p * per_prefill + 4 * li + 4]
            last = li + 1 == len(layers)
            assert [g[0] for g in got] == ["gemm_wfp4", "gemm_wfp4_norm", "gemm_wfp4", "gemm_wfp4" if last else "gemm_wfp4_norm"]
            for g, name in zip(got, ("qkv_w", "o_w", "gu_w", "down_w")):
                assert g[1] is lw[name + "4"] and g[2] is lw[name + "_s4"], (li, name)
                assert g[1].dtype == torch.uint8 and g[2].dtype == torch.uint8
    # the bf16 GEMMs that remain are the vision tower's and the merger's: none reads a language-model matrix
    lm = {id(t) for lw in layers for t in lw.values() if torch.is_tensor(t)}
    assert not [c for c in ops.calls if c[0] == "gemm" and id(c[1]) in lm]
    assert eng._fp8_scratch is None and eng._fp8_scratch_owner._fp8_scratch is None
    # ... while the scratch engine of the same weights does dequantise, four matrices per layer and prefill
    ops2 = Recording()
    scratch = _model(cfg, sd, ops2, llm_fp4=True)
    ops2.calls.clear()
    H.run_engine_stream(scratch, 1)
    assert [c[0] for c in ops2.calls].count("dequant_fp4") == 4 * len(layers) and scratch._svlm_engine._fp8_scratch is not None
    assert not [c for c in ops2.calls if c[0].startswith("gemm_wfp4")]


def test_prefill_fp4_refusals():
    assert FP4_PREFILL_OPS == ("gemm_wfp4", "gemm_wfp4_norm") and "dequant_fp4" in FP4_LLM_OPS
    cfg = C.tiny()
    sd = random_state_dict(cfg, 0, "cpu")
    with pytest.raises(ValueError, match="needs llm_fp4=True"):
        _model(cfg, sd, RefOpsWfp4(), prefill_fp4=True)
    with pytest.raises(ValueError, match="needs llm_fp4=True"):
        _model(cfg, sd, RefOpsWfp4(), llm_fp8=True, prefill_fp4=True)
    with pytest.raises(ValueError, match="weight-fp4 GEMMs.*gemm_wfp4"):
        _model(cfg, sd, RefOpsFp4(), llm_fp4=True, prefill_fp4=True)
    odd = C.tiny()
    odd.text.intermediate_size = 544          # a multiple of 32 (llm_fp4 takes it), not of 64
    with pytest.raises(ValueError, match="multiple of 64.*intermediate is 544"):
        _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsWfp4(), llm_fp4=True, prefill_fp4=True)
    assert _model(odd, random_state_dict(odd, 0, "cpu"), RefOpsWfp4(), llm_fp4=True)._svlm_engine.prefill_fp4 is False
    # engines that share weights must agree on the flag
    base = _model(cfg, sd, RefOpsWfp4(), llm_fp4=True, prefill_fp4=True)._svlm_engine
    with pytest.raises(ValueError, match="prefill_fp4"):
        SvlmEngine(cfg, None, "cpu", llm_fp4=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    lane = SvlmEngine(cfg, None, "cpu", llm_fp4=True, prefill_fp4=True, share=base, max_len=1024, max_new_tokens=8, use_graph=False)
    assert lane.prefill_fp4 and lane.w is base.w
    # a stream group still refuses every llm_fp4 engine
    with pytest.raises(ValueError, match="llm_fp4"):
        StreamGroup(base, 2)


def test_header_declares_and_the_ctypes_table_binds_both_entries():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from streaming_vlm_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))
    twins = {"svlm_gemm_wfp4": "svlm_gemm_wfp8", "svlm_gemm_wfp4_norm": "svlm_gemm_wfp8_norm"}
    args = lambda n: [a.strip() for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()]
    for n, twin in twins.items():
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES and getattr(lib, n)
        assert len(args(n)) == len(_lib.SIGNATURES[n][1]), n
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[twin], "the wfp8 twin's argument list"
        # ... name by name, but for the weight operand and its scales (a const void*: e8m0 bytes, not floats)
        want = [a.replace("W8", "W4").replace("const float* w_scale", "const void* w_scale") for a in args(twin)]
        assert args(n) == want, (n, args(n), want)
    assert _lib.load().svlm_abi_version() == 1


def _host_plan(lib, M, N, K, act, norm, env):
    with H.forced_switches(env):          # goes to the C environment the diagnostic library reads
        v = (ctypes.c_int * 10)()
        lib.svlm_diag_last_gemm_plan(v, 10)
        seq = v[0]
        fake = ctypes.c_void_p(4096)
        a = [fake, K, fake, K // 2, fake, None, None, 0, fake, N, M, N, K, act, fake, P.WS_BYTES]
        if norm:
            lib.svlm_gemm_wfp4_norm(*a, fake, None, 1e-6, fake, N, None)
        else:
            lib.svlm_gemm_wfp4(*a, None)
        lib.svlm_diag_last_gemm_plan(v, 10)
        assert v[0] == seq + 1, f"the call was rejected before it planned: {lib.svlm_last_error()}"
        return dict(fp8=v[1], bm=v[2], waves=v[3], stages=v[4], dma=v[5], splits=v[6], kps=v[7], table=v[8])


def test_wfp4_mirror_matches_the_library_plan():
    """The diagnostic library notes the plan of a svlm_gemm_wfp4 call before it touches the device (the technique of
    tests/test_prefill_fp8_host.py::test_wfp8_mirror_matches_the_library_plan), so tests/gemm_wfp4_paths.py:plan_wfp4 is pinned to
    gemm_wfp4_impl without a GPU: every case of the GPU test and a grid of shapes around the table buckets and the large-M rule.  The
    plan is also the plan of the weight-fp8 GEMM, so that a prefill_fp4 engine keeps the scratch path's K per split."""
    if torch.cuda.is_available():
        pytest.skip("GPU present: tests/test_gemm_wfp4_gpu.py asserts the reported plan of real launches instead")
    import gemm_wfp8_paths as P8
    from test_gemm_ref64 import _diag_lib
    lib = _diag_lib()
    n = 0
    for c in P.CASES:
        want = P.plan_wfp4(c["M"], c["N"], c["K"], act=c["act"], norm=c["norm"] is not None, env=c["force"])
        got = _host_plan(lib, c["M"], c["N"], c["K"], c["act"], c["norm"] is not None, c["force"])
        assert got == {k: want[k] for k in got}, (c["id"], got, want)
        n += 1
    shapes = [(N, K) for (_, N, K, _, _) in P.TUNED] + [(2048, 1536), (1536, 1536), (8960, 1536), (260, 4096), (1024, 256)]
    for N, K in shapes:
        for M in (1, 64, 65, 191, 192, 193, 256, 275, 290, 384, 385, 448, 449, 512, 590, 704, 705, 2047, 2048, 2305, 4096):
            for act in ((0, 4) if N % 8 == 0 else (0,)):
                want = P.plan_wfp4(M, N, K, act=act)
                got = _host_plan(lib, M, N, K, act, False, None)
                assert got == {k: want[k] for k in got}, (M, N, K, act, got, want)
                w8 = P8.plan_wfp8(M, N, K, act=act)
                assert all(want[k] == w8[k] for k in ("bm", "waves", "stages", "splits", "kps", "table")), (M, N, K, act)
                n += 1
    assert n > 300 and got["fp8"] == 3
    # the three switches, one by one
    for env in ({"SVLM_GEMM_WFP4_NO_TABLE": "1"}, {"SVLM_GEMM_WFP4_BM": "128"}, {"SVLM_GEMM_WFP4_BM": "256", "SVLM_GEMM_WFP4_SPLITS": "5"}):
        want = P.plan_wfp4(290, 3584, 18944, env=env)
        got = _host_plan(lib, 290, 3584, 18944, 0, False, env)
        assert got == {k: want[k] for k in got}, (env, got, want)
    assert P.plan_wfp4(290, 3584, 18944, env={"SVLM_GEMM_WFP4_NO_TABLE": "1"})["table"] == 0 != P.plan_wfp4(290, 3584, 18944)["table"]


def test_passes_above_the_row_threshold_go_through_the_scratch_layer():
    """`PREFILL_FP4_MAX_ROWS`: a pass of more rows dequantises and runs the bf16 GEMMs (the dense prefill's 4096-row passes); same model,
    same bits.  The threshold is lowered on one engine so that the tiny stream's prefills (tens of rows) cross it."""
    assert SvlmEngine.PREFILL_FP4_MAX_ROWS == 1024 < SvlmEngine.PREFILL_ROWS
    cfg = C.tiny()
    sd = H.decisive_weights(cfg)
    ops = Recording()
    model = _model(cfg, sd, ops, llm_fp4=True, prefill_fp4=True)
    model._svlm_engine.PREFILL_FP4_MAX_ROWS = 8
    ops.calls.clear()
    got = H.run_engine_stream(model, 2, keep_logits=True)
    names = [c[0] for c in ops.calls]
    assert names.count("dequant_fp4") == 4 * len(model._svlm_engine.w.layers) * 2 and not [n for n in names if n.startswith("gemm_wfp4")]
    assert model._svlm_engine._fp8_scratch is not None
    want = H.run_engine_stream(_model(cfg, sd, RefOpsWfp4(), llm_fp4=True, prefill_fp4=True), 2, keep_logits=True)
    assert got[1] == want[1] and [e["ids"] for e in got[3]] == [e["ids"] for e in want[3]]
    for a, b in zip(got[3], want[3]):
        assert torch.equal(torch.stack(a["logits"]), torch.stack(b["logits"]))


# ------------------------------------------------------------------------------------------------ torch emulation of the tile loop
FAULTS = ("next_block", "next_row", "prev_ktile", "no_k_begin", "swapped_nibbles")
_LUT = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32)


def emulate(A, W4, s, plan, fault=None):
    """What gemm_wfp4_kernel computes for C = A . W'^T, addressed as the kernel addresses it: per K-split (k_begin = split * kps), per
    K-tile kt of 64 and K-step ks of 32, lane group fq reads the 4 bytes at row * ldw + k_begin / 2 + kt * 32 + ks * 16 + fq * 4 (8
    codes, element 2i in the low nibble of byte i) and the scale byte at row * (K / 32) + k_begin / 32 + 2 kt + ks; code * 2^e in
    bf16, products accumulated in fp32 per split, the splits summed in fp32, one rounding to bf16.  `fault`: one of FAULTS."""
    N, K = W4.shape[0], W4.shape[1] * 2
    nb = K // 32
    raw4, raws = W4.reshape(-1), s.reshape(-1)
    rows = torch.arange(N)
    Af = A.float()
    out = torch.zeros((A.shape[0], N), dtype=torch.float32)
    for split in range(plan["splits"]):
        k_begin = split * plan["kps"]
        k_end = min(K, k_begin + plan["kps"])
        part = torch.zeros_like(out)
        for kt in range((k_end - k_begin) // 64):
            for ks in range(2):
                sidx = ((0 if fault == "no_k_begin" else k_begin // 32) + 2 * kt + ks + (1 if fault == "next_block" else 0)
                        - (2 if fault == "prev_ktile" else 0)) % nb
                srow = (rows + 1) % N if fault == "next_row" else rows
                scale = torch.pow(2.0, raws[srow * nb + sidx].float() - 127)                   # [N]
                frag = torch.empty((N, 32), dtype=torch.float32)
                for fq in range(4):
                    byte = raw4[(rows * (K // 2) + k_begin // 2 + kt * 32 + ks * 16 + fq * 4)[:, None] + torch.arange(4)[None, :]]    # [N, 4]
                    lo, hi = _LUT[(byte & 0xF).long()], _LUT[(byte >> 4).long()]
                    pair = torch.stack([hi, lo] if fault == "swapped_nibbles" else [lo, hi], dim=-1)
                    frag[:, fq * 8:fq * 8 + 8] = pair.view(N, 8)
                wb = (frag * scale[:, None]).to(BF16).float()                                  # the MFMA's bf16 operand
                k0 = k_begin + kt * 64 + ks * 32
                part += Af[:, k0:k0 + 32] @ wb.t()
        out += part
    return out.to(BF16)


def _emulated_cases():
    for c in P.SMALL_BLOCKS:
        o = P.operands("blocks", c["M"], c["N"], c["K"])
        plan = P.plan_wfp4(c["M"], c["N"], c["K"], env=c["force"])
        ref, bound, _, _ = R.reference(o["A"], o["Wp"], c=R.fadds(dict(plan, fp8=0), c["K"]))
        yield c, o, plan, ref, bound


def test_tile_loop_emulation_meets_the_bound_and_every_injected_fault_exceeds_it():
    """The emulation is exact on every small `blocks` case (one product per output), so it is inside the bound; each of the five
    faults the generator is built to expose (scale of the next block, of the next row, of the previous K-tile, scale index that
    ignores k_begin, swapped nibbles) exceeds the bound on at least one of them -- the ones that need a K-split only there."""
    assert len(P.SMALL_BLOCKS) >= 12 and any(P.plan_wfp4(c["M"], c["N"], c["K"], env=c["force"])["splits"] > 1 for c in P.SMALL_BLOCKS)
    caught = {f: [] for f in FAULTS}
    for c, o, plan, ref, bound in _emulated_cases():
        got = emulate(o["A"], o["W4"], o["s"], plan)
        ratio, _ = R.ratios(got, ref, bound)
        assert float(ratio.max()) <= 1.0 and bool((got.double() == ref).all()), c["id"]
        for f in FAULTS:
            if f == "no_k_begin" and plan["splits"] == 1:
                continue
            ratio, _ = R.ratios(emulate(o["A"], o["W4"], o["s"], plan, fault=f), ref, bound)
            if float(ratio.max()) > 1.0:
                caught[f].append(c["id"])
    print({f: len(v) for f, v in caught.items()})
    assert all(caught[f] for f in FAULTS), {f: len(v) for f, v in caught.items()}
