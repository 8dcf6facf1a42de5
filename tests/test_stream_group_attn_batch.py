"""Stream groups with batched_attn=True (svlm_decb_attn, csrc/decode_attn.hip) without a GPU: the ABI of the entry and its record, which
entries one step issues with and without the flag in all four step forms (a recording ops backend stands in for the GPU, as in
tests/test_stream_group_wide.py), the refusal and the pass-through of the keyword."""
import ctypes
import inspect
import os
import re
from types import SimpleNamespace

import pytest
import torch

from streaming_vlm_amd import stream_group as SG
from streaming_vlm_amd.stream_group import StreamGroup
from test_stream_group_wide import RecordingOps, _built, _fake_engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["svlm_decb_attn", "svlm_decb_attn_max_lanes"]


def test_the_entry_is_declared_exported_bound_and_wrapped():
    lib = _built()
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    for n in ENTRIES:
        assert re.search(r"\b%s\s*\(" % n, hdr), f"{n} is not declared in include/svlm.h"
        assert n in _lib.SIGNATURES, f"{n} is not in _lib.SIGNATURES"
        assert getattr(lib, n)
        args = [a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip() and a.strip() != "void"]
        assert len(args) == len(_lib.SIGNATURES[n][1]), n
        assert callable(getattr(HipOps, n[len("svlm_"):])), f"ops.py has no wrapper for {n}"
    assert callable(HipOps.lane_attn_record)
    assert lib.svlm_decb_attn_max_lanes() == 16 == SG.MAX_LANES_WIDE
    assert "decb_attn" in SG.ATTN_GROUP_OPS


def test_the_record_is_mirrored_at_the_size_the_packer_writes():
    from streaming_vlm_amd.ops import HipOps
    hdr = open(os.path.join(ROOT, "include", "svlm.h")).read()
    body = re.search(r"typedef struct svlm_lane_attn \{(.*?)\} svlm_lane_attn;", hdr, flags=re.S).group(1)
    fields = [f.strip() for f in re.sub(r"/\*.*?\*/", "", body, flags=re.S).split(";") if f.strip()]
    size = sum(8 if "*" in f else 4 for f in fields)              # pointers first, then ints: no padding
    assert [f.split()[-1].lstrip("*") for f in fields] == ["rope_cs", "lin_len_dev", "ws", "attn_len", "chunk"]
    assert size == 32 == HipOps.ATTN_WORDS * 8
    mirror = open(os.path.join(ROOT, "streaming-vlm_amd", "csrc", "dec_lanes.h")).read()
    assert re.search(r"static_assert\(sizeof\(svlm_lane_attn\) == 32", mirror)
    # the lane record it goes with is unchanged
    assert HipOps.LANE_WORDS * 8 == 72 and re.search(r"static_assert\(sizeof\(svlm_lane\) == 72", mirror)


def test_the_host_checks_of_the_library_need_no_gpu():
    """B, the tables, the head shape and every lane's chunk are refused before anything is launched."""
    lib = _built()
    lib.svlm_decb_attn.restype = ctypes.c_int
    lib.svlm_decb_attn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_void_p, ctypes.c_void_p]
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)

    def call(lanes=p, attn=p, B=2, Hq=12, Hkv=2, D=128, chunks=(48, 48), ldq=1536):
        host = (ctypes.c_int * 6)(1024, 1024, chunks[0], chunks[1], 0, 0)
        h = ctypes.addressof(host)
        return lib.svlm_decb_attn(lanes, attn, B, p, ldq, p, 1536, 0, Hq, Hkv, D, 0.1, h, h + 8, h + 16, None)

    for kw in (dict(B=0), dict(B=17), dict(lanes=None), dict(attn=None), dict(Hq=9, Hkv=1), dict(Hq=12, Hkv=5), dict(D=64),
               dict(chunks=(48, 24)), dict(chunks=(80, 48)), dict(chunks=(48, 576)), dict(chunks=(0, 48)), dict(ldq=1530), dict(ldq=1024)):
        assert call(**kw) != 0, kw


# ----------------------------------------------------------------------------- which entries a step issues
def _step(B, form, batched_attn):
    """One `_step_launch` of a group object that skipped the GPU allocations of __init__; form: bf16, fp8, fp4 or wide."""
    ops = RecordingOps()
    group = StreamGroup.__new__(StreamGroup)
    group.engine = _fake_engine(ops, llm_fp8=form == "fp8", llm_fp4=form == "fp4")
    for lw in group.engine.w.layers:
        for k in ("qkv_w8", "qkv_w_s", "o_w8", "o_w_s", "gu_w8", "gu_w_s", "down_w8", "down_w_s", "qkv_w4", "qkv_w_s4", "o_w4", "o_w_s4", "gu_w4",
                  "gu_w_s4", "down_w4", "down_w_s4"):
            lw[k] = lw["ln1"][:3] + k
    group.engine.w.lm_head8, group.engine.w.lm_head_s = "lm_head8", "lm_head_s"
    group.wide, group.sampling = form == "wide", False
    if batched_attn is not None:                      # (None: a group object from before the option existed)
        group.batched_attn = batched_attn
    group.table, group.samples, group.x, group.h, group.logits, group.ws, group.suppress = "tab", None, "x", "h", "logits", "ws", "sup"
    group.q, group.attn, group.attn_table = "q", "attn", "attn_tab"
    group._attn_host_args = ([64 + j for j in range(B)], [32] * B, [False] * B)
    if not batched_attn:
        group.q, group.attn = [f"q{j}" for j in range(B)], [f"a{j}" for j in range(B)]
    act = [(SimpleNamespace(rope_cs=f"rope{j}", d_ws=f"dws{j}", _attn_len=64 + j, decode_chunk=32, state=[0, 0]),
            SimpleNamespace(pool=f"pool{j}", slot_of_dev=f"slots{j}")) for j in range(B)]
    group._step_launch(act, False)
    return ops.calls


@pytest.mark.parametrize("form", ["bf16", "fp8", "fp4", "wide"])
@pytest.mark.parametrize("B", [1, 3])
def test_a_step_with_the_flag_issues_one_decb_attn_per_layer(form, B):
    plain, flag = _step(B, form, False), _step(B, form, True)
    names_p, names_f = [c[0] for c in plain], [c[0] for c in flag]
    assert names_f.count("decb_attn") == 2 and "decode_attn" not in names_f          # two layers
    assert names_p.count("decode_attn") == 2 * B and "decb_attn" not in names_p
    # the other entries: unchanged and in the same order, each run of B decode_attn calls replaced by one decb_attn
    collapsed = []
    for n in names_p:
        if n == "decode_attn":
            if collapsed[-1] != "decb_attn":
                collapsed.append("decb_attn")
        else:
            collapsed.append(n)
    assert names_f == collapsed
    others_p = [c for c in plain if c[0] != "decode_attn"]
    others_f = [c for c in flag if c[0] != "decb_attn"]
    for (n1, a1, k1), (n2, a2, k2) in zip(others_p, others_f):
        if "q0" in repr(a1) or "a0" in repr(a1):       # (the fake per-lane q / attn rows of the looped form stand for the same buffers)
            continue
        assert (n1, a1, k1) == (n2, a2, k2)
    for li, (n, a, kw) in enumerate(c for c in flag if c[0] == "decb_attn"):
        assert a == ("tab", "attn_tab", B, "q", "attn", li, 4, 1.0 / 128 ** 0.5, [64 + j for j in range(B)], [32] * B, [False] * B, 2, 128) and not kw


@pytest.mark.parametrize("form", ["bf16", "fp8", "fp4", "wide"])
def test_without_the_flag_the_sequence_is_todays(form):
    pre = {"bf16": "decb_", "fp8": "decb_", "fp4": "decb_", "wide": "decw_"}[form]
    sfx = {"bf16": "", "fp8": "_fp8", "fp4": "_fp4", "wide": ""}[form]
    head = ["decb_lm_head_fp8" if form in ("fp8", "fp4") else pre + "lm_head", pre + "argmax_finish"]
    per_layer = [pre + "qkv" + sfx] + ["decode_attn"] * 3 + [pre + "gemv" + sfx, pre + "gate_up" + sfx, pre + "gemv" + sfx]
    want = [pre + "embed"] + per_layer * 2 + head
    assert [c[0] for c in _step(3, form, False)] == want
    assert [c[0] for c in _step(3, form, None)] == want
    a = [c for c in _step(3, form, False) if c[0] == "decode_attn"][4]         # layer 1, lane 1: its own rows, pool, tables and workspace
    assert a[1][:10] == ("q1", "pool1", 1, "slots1", "rope1", "a1", "dws1", 4, 65, 32)


# ----------------------------------------------------------------------------- the option itself
def test_a_backend_without_the_entry_is_refused_by_name():
    for missing in (("decb_attn",), ("lane_attn_record",), SG.ATTN_GROUP_OPS):
        with pytest.raises(ValueError, match=r"batched_attn=True.*lane-batched attention") as ei:
            StreamGroup(_fake_engine(RecordingOps(without=missing)), 2, batched_attn=True)
        assert all(m in str(ei.value) for m in missing), str(ei.value)
    with pytest.raises(ValueError, match=r"batched_attn=True"):
        StreamGroup(_fake_engine(RecordingOps(without=("decb_attn",))), 2, wide=True, batched_attn=True)


def test_the_table_is_allocated_only_with_the_flag(monkeypatch):
    monkeypatch.setattr(SG, "SvlmEngine", lambda *a, **k: SimpleNamespace())

    class Ops(RecordingOps):
        ATTN_WORDS = 4

    group = StreamGroup(_fake_engine(Ops()), 3, batched_attn=True)
    assert group.batched_attn and tuple(group.attn_table.shape) == (3, 4) == tuple(group._attn_table_host.shape)
    assert group.attn_table.dtype == torch.int64
    wide = StreamGroup(_fake_engine(Ops()), 16, wide=True, batched_attn=True)
    assert wide.wide and tuple(wide.attn_table.shape) == (16, 4)
    plain = StreamGroup(_fake_engine(RecordingOps(without=SG.ATTN_GROUP_OPS)), 3)          # without the flag the entry is not needed
    assert not plain.batched_attn and plain.attn_table is None


def test_the_group_api_passes_the_flag_through(monkeypatch):
    from streaming_vlm_amd import multi_stream
    assert inspect.signature(multi_stream.streaming_inference_group).parameters["batched_attn"].default is False
    assert inspect.signature(StreamGroup.__init__).parameters["batched_attn"].default is False
    seen = {}

    class FakeGroup:
        n_lanes = 1

        def __init__(self, engine, n_lanes, **kw):
            seen.update(n_lanes=n_lanes, **kw)
            raise RuntimeError("stop here")

    monkeypatch.setattr(SG, "StreamGroup", FakeGroup)
    with pytest.raises(RuntimeError, match="stop here"):
        multi_stream.streaming_inference_group(SimpleNamespace(_svlm_engine=None), None, [{}] * 5, n_lanes=5, wide=True, batched_attn=True)
    assert seen == dict(n_lanes=5, sampling=False, wide=True, batched_attn=True)
    seen.clear()
    with pytest.raises(RuntimeError, match="stop here"):
        multi_stream.streaming_inference_group(SimpleNamespace(_svlm_engine=None), None, [{}] * 2)
    assert seen == dict(n_lanes=2, sampling=False, wide=False)          # off: exactly the call of before
