"""Stream groups on an llm_fp4 engine without a GPU: the ABI of the lane-batched fp4 entries, the refusal of an ops backend that lacks
them (or the batched fp8 head an fp4 engine's e4m3 lm_head needs), and which entries one batched step issues on which tensors (a
recording ops backend stands in for the GPU)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from streaming_vlm_amd import stream_group as SG
from streaming_vlm_amd.stream_group import StreamGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP4_ENTRIES = ["svlm_decb_qkv_fp4", "svlm_decb_gate_up_fp4", "svlm_decb_gemv_fp4"]
BF16_OPS = ("decb_qkv", "decb_gate_up", "decb_gemv", "decb_lm_head", "decb_lm_head_sample")
FP8_LAYER_OPS = ("decb_qkv_fp8", "decb_gate_up_fp8", "decb_gemv_fp8")


def test_batched_fp4_entry_points_are_declared_exported_and_bound():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))
    for n in FP4_ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, hdr), f"{n} is not declared in include/svlm.h"
        assert n in _lib.SIGNATURES, f"{n} is not in _lib.SIGNATURES"
        assert getattr(lib, n)
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[n][1]), n
        assert callable(getattr(HipOps, n[len("svlm_"):])), f"ops.py has no wrapper for {n}"
    # signatures are the fp8 twins' (w_scale is a pointer in both bindings)
    for n in FP4_ENTRIES:
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n[:-1] + "8"], n
    assert [("svlm_" + m) for m in SG.FP4_GROUP_OPS] == FP4_ENTRIES + ["svlm_decb_lm_head_fp8"]
    # the lane table did not change
    assert HipOps.LANE_WORDS * 8 == 72
    fields = re.search(r"typedef struct svlm_lane \{(.*?)\} svlm_lane;", hdr, flags=re.S).group(1)
    assert sum(8 if "*" in f else 4 for f in fields.split(";") if f.strip()) == 72


class RecordingOps:
    """Notes the name and arguments of every entry a step issues; `without`: entry points this backend does not have."""

    def __init__(self, without=()):
        self.calls = []
        self._without = set(without)

    def __getattr__(self, name):
        if name.startswith("_") or name in self._without:
            raise AttributeError(name)

        def record(*args, **kw):
            self.calls.append((name, args, kw))
        return record


def _fake_fp4_engine(ops, n_layers=2):
    keys = ("ln1", "ln2", "qkv_b", "qkv_w4", "qkv_w_s4", "o_w4", "o_w_s4", "gu_w4", "gu_w_s4", "down_w4", "down_w_s4")
    layers = [{k: f"L{li}.{k}" for k in keys} for li in range(n_layers)]
    w = SimpleNamespace(embed="embed", final_norm="final_norm", lm_head=None, lm_head8="lm_head8", lm_head_s="lm_head_s", layers=layers)
    text = SimpleNamespace(head_dim=128, rms_eps=1e-6, num_heads=4, vocab_size=1000)
    return SimpleNamespace(llm_fp8=False, llm_fp4=True, prefill_fp4=False, decode_tail=False, ops=ops, w=w, cfg=SimpleNamespace(text=text),
                           qd=512, kd=256)


def test_fp4_engine_without_the_batched_entries_is_refused():
    fp4_ops = SG.FP4_GROUP_OPS
    for missing in (fp4_ops, fp4_ops[2:3], fp4_ops[0:1], fp4_ops[3:4]):
        with pytest.raises(ValueError, match="llm_fp4") as ei:
            StreamGroup(_fake_fp4_engine(RecordingOps(without=missing)), 2)
        assert all(m in str(ei.value) for m in missing), str(ei.value)
        # what the backend has is not listed as missing
        assert not any(re.search(r"'%s'" % m, str(ei.value)) for m in fp4_ops if m not in missing), str(ei.value)


def test_sampling_fp4_group_without_the_fp8_sampling_head_is_refused():
    with pytest.raises(ValueError, match="llm_fp4") as ei:
        StreamGroup(_fake_fp4_engine(RecordingOps(without=("decb_lm_head_sample_fp8",))), 2, sampling=True)
    assert "decb_lm_head_sample_fp8" in str(ei.value)


def _step(sampled, B=2):
    ops = RecordingOps()
    eng = _fake_fp4_engine(ops)
    # the step alone, on a group object that skipped the GPU allocations of __init__
    group = StreamGroup.__new__(StreamGroup)
    group.engine = eng
    group.table, group.samples, group.x, group.h, group.logits, group.ws, group.suppress = "tab", "smp", "x", "h", "logits", "ws", "sup"
    group.q, group.attn = [f"q{j}" for j in range(B)], [f"a{j}" for j in range(B)]
    lane = SimpleNamespace(rope_cs="rope", d_ws="dws", _attn_len=64, decode_chunk=32, state=[0, 0])
    cache = SimpleNamespace(pool="pool", slot_of_dev="slots")
    group._step_launch([(lane, cache)] * B, sampled)
    return ops.calls


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("sampled", [False, True])
def test_step_of_an_fp4_group_issues_the_fp4_entries_and_the_fp8_head(sampled, B):
    names = [c[0] for c in _step(sampled, B)]
    assert not any(n in BF16_OPS for n in names), f"a bf16 lane-batched entry was issued on an fp4 engine: {names}"
    assert not any(n in FP8_LAYER_OPS for n in names), f"an fp8 layer entry was issued on an fp4 engine: {names}"
    per_layer = ["decb_qkv_fp4"] + ["decode_attn"] * B + ["decb_gemv_fp4", "decb_gate_up_fp4", "decb_gemv_fp4"]
    tail = ["decb_lm_head_sample_fp8", "decb_sample_finish"] if sampled else ["decb_lm_head_fp8", "decb_argmax_finish"]
    assert names == ["decb_embed"] + per_layer * 2 + tail
    assert names.count("decb_embed") == 1


def test_step_of_an_fp4_group_passes_each_layers_codes_and_block_scales():
    by_name = {}
    for n, args, _ in _step(False):
        by_name.setdefault(n, []).append(args)
    for li in range(2):
        qkv = by_name["decb_qkv_fp4"][li]
        assert qkv[:2] == ("tab", 2) and qkv[2:4] == ("x", f"L{li}.ln1")
        assert (f"L{li}.qkv_w4", f"L{li}.qkv_w_s4", f"L{li}.qkv_b") == qkv[5:8] and qkv[9] == li
        o, down = by_name["decb_gemv_fp4"][2 * li], by_name["decb_gemv_fp4"][2 * li + 1]
        assert o[3:5] == (f"L{li}.o_w4", f"L{li}.o_w_s4") and down[3:5] == (f"L{li}.down_w4", f"L{li}.down_w_s4")
        assert o[5:] == ("x", "x") and down[2] == "h" and down[5:] == ("x", "x")
        gu = by_name["decb_gate_up_fp4"][li]
        assert gu[2:4] == ("x", f"L{li}.ln2") and gu[5:8] == (f"L{li}.gu_w4", f"L{li}.gu_w_s4", "h")
    head = by_name["decb_lm_head_fp8"][0]
    assert head[3] == "final_norm" and head[5:7] == ("lm_head8", "lm_head_s") and head[7:] == ("logits", "sup", "ws")
    assert by_name["decb_embed"][0] == ("tab", 2, "embed", "x")
    assert by_name["decb_argmax_finish"][0][:3] == ("tab", 2, "ws")


def test_sampled_step_of_an_fp4_group_passes_the_sample_table_to_the_fp8_head():
    by_name = {}
    for n, args, _ in _step(True):
        by_name.setdefault(n, []).append(args)
    head = by_name["decb_lm_head_sample_fp8"][0]
    assert head[:3] == ("tab", "smp", 2) and head[4] == "final_norm" and head[6:8] == ("lm_head8", "lm_head_s")
    assert by_name["decb_sample_finish"][0][:3] == ("tab", "smp", 2)
