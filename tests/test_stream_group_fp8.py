"""Stream groups on an llm_fp8 engine without a GPU: the ABI of the lane-batched fp8 entries, the refusal of an ops backend that lacks
them, and which entries one batched step issues (a recording ops backend stands in for the GPU)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest

from streaming_vlm_amd.stream_group import FP8_GROUP_OPS, StreamGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP8_ENTRIES = ["svlm_decb_qkv_fp8", "svlm_decb_gate_up_fp8", "svlm_decb_gemv_fp8", "svlm_decb_lm_head_fp8"]
BF16_OPS = ("decb_qkv", "decb_gate_up", "decb_gemv", "decb_lm_head")


def test_batched_fp8_entry_points_are_declared_exported_and_bound():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))
    for n in FP8_ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, hdr), f"{n} is not declared in include/svlm.h"
        assert n in _lib.SIGNATURES, f"{n} is not in _lib.SIGNATURES"
        assert getattr(lib, n)
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[n][1]), n
        assert callable(getattr(HipOps, n[len("svlm_"):])), f"ops.py has no wrapper for {n}"
    assert [("svlm_" + m) for m in FP8_GROUP_OPS] == FP8_ENTRIES
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


def _fake_fp8_engine(ops, n_layers=2):
    layers = [{k: f"L{li}.{k}" for k in ("ln1", "ln2", "qkv_b", "qkv_w8", "qkv_w_s", "o_w8", "o_w_s", "gu_w8", "gu_w_s", "down_w8", "down_w_s")}
              for li in range(n_layers)]
    w = SimpleNamespace(embed="embed", final_norm="final_norm", lm_head=None, lm_head8="lm_head8", lm_head_s="lm_head_s", layers=layers)
    text = SimpleNamespace(head_dim=128, rms_eps=1e-6, num_heads=4, vocab_size=1000)
    return SimpleNamespace(llm_fp8=True, decode_tail=False, ops=ops, w=w, cfg=SimpleNamespace(text=text), qd=512, kd=256)


def test_fp8_engine_without_the_batched_fp8_entries_is_refused():
    for missing in (FP8_GROUP_OPS, FP8_GROUP_OPS[2:3]):
        with pytest.raises(ValueError, match="llm_fp8") as ei:
            StreamGroup(_fake_fp8_engine(RecordingOps(without=missing)), 2)
        assert all(m in str(ei.value) for m in missing)


def test_step_of_an_fp8_group_issues_the_fp8_entries_on_the_fp8_tensors():
    ops = RecordingOps()
    eng = _fake_fp8_engine(ops)
    # the step alone, on a group object that skipped the GPU allocations of __init__
    group = StreamGroup.__new__(StreamGroup)
    group.engine = eng
    group.table, group.x, group.q, group.attn, group.h, group.logits, group.ws, group.suppress = "tab", "x", ["q0", "q1"], ["a0", "a1"], "h", "logits", "ws", "sup"
    lane = SimpleNamespace(rope_cs="rope", d_ws="dws", _attn_len=64, decode_chunk=32, state=[0, 0])
    cache = SimpleNamespace(pool="pool", slot_of_dev="slots")
    group._step_launch([(lane, cache), (lane, cache)])
    names = [c[0] for c in ops.calls]
    assert not any(n in BF16_OPS for n in names), f"a bf16 lane-batched entry was issued on an fp8 engine: {names}"
    per_layer = ["decb_qkv_fp8", "decode_attn", "decode_attn", "decb_gemv_fp8", "decb_gate_up_fp8", "decb_gemv_fp8"]
    assert names == ["decb_embed"] + per_layer * 2 + ["decb_lm_head_fp8", "decb_argmax_finish"]
    by_name = {}
    for n, args, _ in ops.calls:
        by_name.setdefault(n, []).append(args)
    for li in range(2):
        qkv = by_name["decb_qkv_fp8"][li]
        assert qkv[:2] == ("tab", 2) and (f"L{li}.qkv_w8", f"L{li}.qkv_w_s", f"L{li}.qkv_b") == qkv[5:8] and qkv[9] == li
        o, down = by_name["decb_gemv_fp8"][2 * li], by_name["decb_gemv_fp8"][2 * li + 1]
        assert o[3:5] == (f"L{li}.o_w8", f"L{li}.o_w_s") and down[3:5] == (f"L{li}.down_w8", f"L{li}.down_w_s")
        assert o[5:] == ("x", "x") and down[2] == "h" and down[5:] == ("x", "x")
        assert by_name["decb_gate_up_fp8"][li][5:7] == (f"L{li}.gu_w8", f"L{li}.gu_w_s")
    head = by_name["decb_lm_head_fp8"][0]
    assert head[3] == "final_norm" and head[5:7] == ("lm_head8", "lm_head_s") and head[7:] == ("logits", "sup", "ws")
    assert by_name["decb_embed"][0] == ("tab", 2, "embed", "x")


def test_step_of_a_bf16_group_is_unchanged():
    ops = RecordingOps()
    eng = _fake_fp8_engine(ops)
    eng.llm_fp8 = False
    for li, lw in enumerate(eng.w.layers):
        lw.update({k: f"L{li}.{k}" for k in ("qkv_w", "o_w", "gu_w", "down_w")})
    eng.w.lm_head = "lm_head"
    group = StreamGroup.__new__(StreamGroup)
    group.engine = eng
    group.table, group.x, group.q, group.attn, group.h, group.logits, group.ws, group.suppress = "tab", "x", ["q0"], ["a0"], "h", "logits", "ws", "sup"
    lane = SimpleNamespace(rope_cs="rope", d_ws="dws", _attn_len=64, decode_chunk=32, state=[0, 0])
    group._step_launch([(lane, SimpleNamespace(pool="pool", slot_of_dev="slots"))])
    names = [c[0] for c in ops.calls]
    per_layer = ["decb_qkv", "decode_attn", "decb_gemv", "decb_gate_up", "decb_gemv"]
    assert names == ["decb_embed"] + per_layer * 2 + ["decb_lm_head", "decb_argmax_finish"]
