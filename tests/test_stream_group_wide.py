"""Wide stream groups (StreamGroup(wide=True), csrc/decode_wide.hip) without a GPU: the ABI of the svlm_decw_* entries, the lane limits
with and without the flag, the refusals, and which entries one wide step issues on which tensors (a recording ops backend stands in for
the GPU, as in tests/test_stream_group_fp4.py)."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from streaming_vlm_amd import stream_group as SG
from streaming_vlm_amd.stream_group import StreamGroup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_ENTRIES = ["svlm_decw_embed", "svlm_decw_qkv", "svlm_decw_gemv", "svlm_decw_gate_up", "svlm_decw_lm_head", "svlm_decw_argmax_finish"]
HOST_ENTRIES = ["svlm_decw_max_lanes", "svlm_decw_plan", "svlm_decw_reserve_lds"]


def _built():
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    return ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))


def test_wide_entry_points_are_declared_exported_and_bound():
    lib = _built()
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    for n in WIDE_ENTRIES + HOST_ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, hdr), f"{n} is not declared in include/svlm.h"
        assert n in _lib.SIGNATURES, f"{n} is not in _lib.SIGNATURES"
        assert getattr(lib, n)
        args = [a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[n][1]), n
        assert callable(getattr(HipOps, n[len("svlm_"):])), f"ops.py has no wrapper for {n}"
    # the wide entries take the arguments of the entries they mirror
    for n in WIDE_ENTRIES:
        assert _lib.SIGNATURES[n] == _lib.SIGNATURES[n.replace("decw", "decb")], n
    assert [("svlm_" + m) for m in SG.WIDE_GROUP_OPS] == WIDE_ENTRIES


def test_max_lanes_and_the_split_plan_are_host_functions():
    lib = _built()
    assert lib.svlm_decw_max_lanes() == 16 == SG.MAX_LANES_WIDE
    assert SG.MAX_LANES == 4 and SG.DEFAULT_LANES == 3

    def plan(fused, K):
        sp, kps = ctypes.c_int(0), ctypes.c_int(0)
        assert lib.svlm_decw_plan(fused, K, ctypes.byref(sp), ctypes.byref(kps)) == 0
        return sp.value, kps.value

    # fused entries: the 4 waves of the norm prologue; gemv: 4 / 8 / 16 waves by the number of 64-wide blocks; whole blocks per wave
    assert plan(1, 1536) == (4, 384) and plan(1, 3584) == (4, 896) and plan(1, 1056) == (4, 320) and plan(1, 8) == (4, 64)
    assert plan(0, 1536) == (8, 192) and plan(0, 8960) == (16, 576) and plan(0, 18944) == (16, 1216) and plan(0, 512) == (4, 128)
    for fused, K in ((0, 1536), (1, 1536), (0, 8960), (0, 2080)):
        sp, kps = plan(fused, K)
        assert sp * kps >= K and kps % 64 == 0
    sp, kps = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.svlm_decw_plan(0, 12, ctypes.byref(sp), ctypes.byref(kps)) != 0          # K must be a multiple of 8


class RecordingOps:
    """Notes the name and arguments of every entry a step issues; `without`: entry points this backend does not have."""
    LANE_WORDS = 9

    def __init__(self, without=()):
        self.calls = []
        self._without = set(without)

    def __getattr__(self, name):
        if name.startswith("_") or name in self._without:
            raise AttributeError(name)

        def record(*args, **kw):
            self.calls.append((name, args, kw))
        return record


def _fake_engine(ops, n_layers=2, llm_fp8=False, llm_fp4=False):
    keys = ("ln1", "ln2", "qkv_w", "qkv_b", "o_w", "gu_w", "down_w")
    layers = [{k: f"L{li}.{k}" for k in keys} for li in range(n_layers)]
    w = SimpleNamespace(embed="embed", final_norm="final_norm", lm_head="lm_head", layers=layers)
    text = SimpleNamespace(head_dim=128, rms_eps=1e-6, num_heads=4, vocab_size=1000, hidden_size=256, intermediate_size=512)
    return SimpleNamespace(llm_fp8=llm_fp8, llm_fp4=llm_fp4, prefill_fp8=False, prefill_fp4=False, decode_tail=False, ops=ops, w=w,
                           cfg=SimpleNamespace(text=text, eos_token_ids=(7, 8)), qd=512, kd=256, device=torch.device("cpu"), max_len=64, max_new=8,
                           _fixed_chunk=None, use_graph=False, kv_slack=0, kv_page_tokens=16, vit_fp8=False, linear_planes=False,
                           default_top_k=1, default_top_p=1.0, eos_dev=None, max_graphs=4)


def test_lane_limits_with_and_without_the_flag(monkeypatch):
    monkeypatch.setattr(SG, "SvlmEngine", lambda *a, **k: SimpleNamespace())      # a lane's engine: nothing of it is used by __init__
    group = StreamGroup(_fake_engine(RecordingOps()), 16, wide=True)
    assert group.wide and group.n_lanes == 16 and len(group.lanes) == 16
    assert tuple(group.x.shape) == (16, 256) and tuple(group.h.shape) == (16, 512) and tuple(group.logits.shape) == (16, 1000)
    assert tuple(group.table.shape) == (16, 9) and tuple(group._table_host.shape) == (32, 9)
    assert StreamGroup(_fake_engine(RecordingOps()), 1, wide=True).n_lanes == 1
    for n in (0, 17):
        with pytest.raises(ValueError, match=r"outside \[1, 16\].*wide=True"):
            StreamGroup(_fake_engine(RecordingOps()), n, wide=True)
    with pytest.raises(ValueError, match=r"outside \[1, 4\]"):
        StreamGroup(_fake_engine(RecordingOps()), 5)
    assert not StreamGroup(_fake_engine(RecordingOps()), 4).wide


def test_wide_refusals_name_the_option():
    with pytest.raises(ValueError, match=r"wide=True.*llm_fp8=True"):
        StreamGroup(_fake_engine(RecordingOps(), llm_fp8=True), 2, wide=True)
    with pytest.raises(ValueError, match=r"wide=True.*llm_fp4=True"):
        StreamGroup(_fake_engine(RecordingOps(), llm_fp4=True), 2, wide=True)
    with pytest.raises(ValueError, match=r"wide=True.*sampling=True"):
        StreamGroup(_fake_engine(RecordingOps()), 2, sampling=True, wide=True)
    for missing in (SG.WIDE_GROUP_OPS, SG.WIDE_GROUP_OPS[2:3], SG.WIDE_GROUP_OPS[4:]):
        with pytest.raises(ValueError, match=r"wide=True.*wide entry points") as ei:
            StreamGroup(_fake_engine(RecordingOps(without=missing)), 2, wide=True)
        assert all(m in str(ei.value) for m in missing), str(ei.value)
        assert not any(re.search(r"'%s'" % m, str(ei.value)) for m in SG.WIDE_GROUP_OPS if m not in missing), str(ei.value)


def _step(B, wide=True):
    ops = RecordingOps()
    group = StreamGroup.__new__(StreamGroup)          # the step alone, on a group object that skipped the GPU allocations of __init__
    group.engine = _fake_engine(ops)
    group.wide, group.sampling = wide, False
    group.table, group.samples, group.x, group.h, group.logits, group.ws, group.suppress = "tab", None, "x", "h", "logits", "ws", "sup"
    group.q, group.attn = [f"q{j}" for j in range(B)], [f"a{j}" for j in range(B)]
    act = [(SimpleNamespace(rope_cs=f"rope{j}", d_ws=f"dws{j}", _attn_len=64, decode_chunk=32, state=[0, 0]),
            SimpleNamespace(pool=f"pool{j}", slot_of_dev=f"slots{j}")) for j in range(B)]
    group._step_launch(act, False)
    return ops.calls


@pytest.mark.parametrize("B", [2, 9])
def test_wide_step_issues_the_wide_entries_in_todays_order(B):
    calls = _step(B)
    names = [c[0] for c in calls]
    per_layer = ["decw_qkv"] + ["decode_attn"] * B + ["decw_gemv", "decw_gate_up", "decw_gemv"]
    assert names == ["decw_embed"] + per_layer * 2 + ["decw_lm_head", "decw_argmax_finish"]
    assert not any(n.startswith("decb_") for n in names)
    by_name = {}
    for n, args, _ in calls:
        by_name.setdefault(n, []).append(args)
    assert by_name["decw_embed"][0] == ("tab", B, "embed", "x")
    for li in range(2):
        assert by_name["decw_qkv"][li] == ("tab", B, "x", f"L{li}.ln1", 1e-6, f"L{li}.qkv_w", f"L{li}.qkv_b", [f"q{j}" for j in range(B)], li, 512,
                                           256, 128, 2)
        for j in range(B):                            # each lane's attention on its own q row, pool, slot table, rope table and workspace
            a = by_name["decode_attn"][li * B + j]
            assert a[:8] == (f"q{j}", f"pool{j}", li, f"slots{j}", f"rope{j}", f"a{j}", f"dws{j}", 4)
        o, down = by_name["decw_gemv"][2 * li], by_name["decw_gemv"][2 * li + 1]
        assert o == ("tab", B, [f"a{j}" for j in range(B)], f"L{li}.o_w", "x", "x")
        assert down == ("tab", B, "h", f"L{li}.down_w", "x", "x")
        assert by_name["decw_gate_up"][li] == ("tab", B, "x", f"L{li}.ln2", 1e-6, f"L{li}.gu_w", "h")
    assert by_name["decw_lm_head"][0] == ("tab", B, "x", "final_norm", 1e-6, "lm_head", "logits", "sup", "ws")
    assert by_name["decw_argmax_finish"][0] == ("tab", B, "ws", 1000, 1)


@pytest.mark.parametrize("B", [1, 4])
def test_a_group_without_the_flag_still_calls_only_decb(B):
    names = [c[0] for c in _step(B, wide=False)]
    assert not any(n.startswith("decw_") for n in names), names
    per_layer = ["decb_qkv"] + ["decode_attn"] * B + ["decb_gemv", "decb_gate_up", "decb_gemv"]
    assert names == ["decb_embed"] + per_layer * 2 + ["decb_lm_head", "decb_argmax_finish"]


def test_group_api_passes_the_flag_through(monkeypatch):
    import inspect
    from streaming_vlm_amd import multi_stream
    assert inspect.signature(multi_stream.streaming_inference_group).parameters["wide"].default is False
    assert inspect.signature(StreamGroup.__init__).parameters["wide"].default is False
    seen = {}

    class FakeGroup:
        n_lanes = 1

        def __init__(self, engine, n_lanes, sampling=False, wide=False):
            seen.update(n_lanes=n_lanes, sampling=sampling, wide=wide)
            raise RuntimeError("stop here")

    monkeypatch.setattr(SG, "StreamGroup", FakeGroup)
    with pytest.raises(RuntimeError, match="stop here"):
        multi_stream.streaming_inference_group(SimpleNamespace(_svlm_engine=None), None, [{}] * 5, n_lanes=5, wide=True)
    assert seen == dict(n_lanes=5, sampling=False, wide=True)
