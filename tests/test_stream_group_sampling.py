"""Per-lane sampling in stream groups without a GPU: which requests a sampling group accepts, the ABI of the three new entries, the
layout of the sampling record, the host's choice of kernel per (top_k, top_p), the refusal of an fp8 backend without the fp8 sampling
head, and which entries a sampled step issues (a recording ops backend stands in for the GPU)."""
import ctypes
import os
import re
import sys
from types import SimpleNamespace

import numpy as np
import pytest

from streaming_vlm_amd.stream_group import FP8_GROUP_OPS, StreamGroup, check_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = {"svlm_decb_lm_head_sample": 16, "svlm_decb_lm_head_sample_fp8": 17, "svlm_decb_sample_finish": 10}


def test_a_sampling_group_accepts_what_generate_begin_accepts_and_the_default_still_refuses():
    ok = dict(ids=[1, 2], cache=None, video_grid_thw=[], max_new_tokens=4)
    for good in (dict(do_sample=True), dict(do_sample=True, top_k=50), dict(do_sample=True, top_k=0, top_p=0.9),
                 dict(do_sample=True, top_k=1), dict(do_sample=False)):
        out = check_request(dict(ok, **good), sampling=True)
        assert all(out[k] == v for k, v in good.items())
    assert "next_vision" not in check_request(dict(ok, do_sample=True, next_vision=(object(), [[1, 2, 2]])), sampling=True)
    for bad in (dict(force_tokens=[3]), dict(keep_logits=True), dict(do_sample=True, top_k=50, keep_logits=True)):
        with pytest.raises(ValueError, match="stream group"):
            check_request(dict(ok, **bad), sampling=True)
    for bad in (dict(do_sample=True), dict(do_sample=True, top_k=50), dict(do_sample=True, top_k=0, top_p=0.9)):
        with pytest.raises(ValueError, match="stream group"):
            check_request(dict(ok, **bad))
        with pytest.raises(ValueError, match="stream group"):
            check_request(dict(ok, **bad), sampling=False)


@pytest.fixture(scope="module")
def built():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    return hdr, ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))


def test_sampling_entry_points_are_declared_exported_and_bound(built):
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    hdr, lib = built
    for n, want in NEW_ENTRIES.items():
        assert re.search(r"\b%s\s*\(" % n, hdr), f"{n} is not declared in include/svlm.h"
        assert n in _lib.SIGNATURES, f"{n} is not in _lib.SIGNATURES"
        assert getattr(lib, n)
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[n][1]) == want, n
        assert callable(getattr(HipOps, n[len("svlm_"):])), f"ops.py has no wrapper for {n}"
    # the fp8 head is the bf16 head with W -> W8, ldw, w_scale; greedy groups on older backends still build
    assert len(_lib.SIGNATURES["svlm_decb_lm_head_sample"][1]) == len(_lib.SIGNATURES["svlm_decb_lm_head"][1]) + 1
    assert "decb_lm_head_sample_fp8" not in FP8_GROUP_OPS and len(FP8_GROUP_OPS) == 4


def test_sampling_record_layout_matches_the_header_and_the_lane_record_is_unchanged(built):
    from streaming_vlm_amd.ops import HipOps
    hdr, _ = built
    fields = re.search(r"typedef struct svlm_lane_sample \{(.*?)\} svlm_lane_sample;", hdr, flags=re.S).group(1)
    names = [f.split()[-1].lstrip("*") for f in fields.split(";") if f.strip()]
    sizes = [8 if "*" in f else 4 for f in fields.split(";") if f.strip()]
    assert names == ["rng", "inv_temp", "top_k", "top_p", "mode"] and sizes == [8, 4, 4, 4, 4]
    assert HipOps.SAMPLE_WORDS * 8 == sum(sizes) == 24
    lane = re.search(r"typedef struct svlm_lane \{(.*?)\} svlm_lane;", hdr, flags=re.S).group(1)
    assert sum(8 if "*" in f else 4 for f in lane.split(";") if f.strip()) == 72 == HipOps.LANE_WORDS * 8
    for name, val in (("GREEDY", 0), ("GUMBEL", 1), ("FILTERED", 2), ("NUCLEUS", 3)):
        assert re.search(r"#define SVLM_SAMPLE_%s %d\b" % (name, val), hdr) and getattr(HipOps, "SAMPLE_" + name) == val
    # a greedy record: null seed, 1/T = 1; the fields land at the header's offsets
    rec = HipOps.lane_sample_record()
    assert rec.dtype == np.int64 and rec.shape == (3,) and rec[0] == 0
    assert rec[1:].view(np.float32)[0] == 1.0 and rec[1:].view(np.int32)[1] == 1 and rec[1:].view(np.int32)[3] == HipOps.SAMPLE_GREEDY
    for bad in (dict(temperature=0.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5)):
        with pytest.raises(Exception, match="lane_sample_record"):
            HipOps.lane_sample_record(**bad)


def test_the_host_picks_the_kernel_by_the_rule_of_penalty_sample():
    from streaming_vlm_amd.ops import HipOps as O
    assert O.sample_mode(1, 1.0) == O.SAMPLE_GREEDY and O.sample_mode(1, 0.5) == O.SAMPLE_GREEDY
    assert O.sample_mode(0, 1.0) == O.SAMPLE_GUMBEL
    assert O.sample_mode(50, 0.9) == O.SAMPLE_FILTERED and O.sample_mode(50, 1.0) == O.SAMPLE_FILTERED
    assert O.sample_mode(2, 1.0) == O.SAMPLE_FILTERED and O.sample_mode(2047, 1.0) == O.SAMPLE_FILTERED
    assert O.sample_mode(0, 0.9) == O.SAMPLE_NUCLEUS
    assert O.sample_mode(4096, 1.0) == O.SAMPLE_NUCLEUS and O.sample_mode(2048, 1.0) == O.SAMPLE_NUCLEUS
    # the rule as csrc/sampling.hip states it (svlm_penalty_sample), branch for branch
    src = open(os.path.join(ROOT, "streaming-vlm_amd", "csrc", "sampling.hip")).read()
    body = src[src.index('extern "C" int svlm_penalty_sample'):]
    order = [body.index("if (top_k == 1)"), body.index("if (top_k == 0 && top_p >= 1.f)"), body.index("if (top_k == 0 || top_k >= SF_CAP)")]
    assert order == sorted(order)
    hdr = open(os.path.join(ROOT, "streaming-vlm_amd", "csrc", "dec_sample.h")).read()
    assert re.search(r"#define SF_CAP 2048\b", hdr)


def test_a_record_that_draws_needs_a_seed_in_device_memory():
    import torch
    from streaming_vlm_amd.ops import HipOps
    for k, p in ((0, 1.0), (50, 0.9), (0, 0.9)):
        with pytest.raises(Exception, match="lane_sample_record"):
            HipOps.lane_sample_record(None, 0.9, k, p)
        with pytest.raises(Exception, match="lane_sample_record.rng: tensor must live on the GPU"):
            HipOps.lane_sample_record(torch.zeros(2, dtype=torch.int32), 0.9, k, p)
    assert HipOps.lane_sample_record(None, 0.9, 1, 0.9)[0] == 0          # top_k = 1 is the argmax: no seed


class RecordingOps:
    """Notes the name and arguments of every entry a step issues; `without`: entry points this backend does not have."""
    SAMPLE_WORDS = 3

    def __init__(self, without=()):
        self.calls = []
        self._without = set(without)

    def __getattr__(self, name):
        if name.startswith("_") or name in self._without:
            raise AttributeError(name)

        def record(*args, **kw):
            self.calls.append((name, args, kw))
        return record


def _fake_engine(ops, fp8, n_layers=2):
    keys = ("ln1", "ln2", "qkv_b", "qkv_w8", "qkv_w_s", "o_w8", "o_w_s", "gu_w8", "gu_w_s", "down_w8", "down_w_s", "qkv_w", "o_w", "gu_w", "down_w")
    layers = [{k: f"L{li}.{k}" for k in keys} for li in range(n_layers)]
    w = SimpleNamespace(embed="embed", final_norm="final_norm", lm_head="lm_head", lm_head8="lm_head8", lm_head_s="lm_head_s", layers=layers)
    text = SimpleNamespace(head_dim=128, rms_eps=1e-6, num_heads=4, vocab_size=1000)
    return SimpleNamespace(llm_fp8=fp8, decode_tail=False, ops=ops, w=w, cfg=SimpleNamespace(text=text), qd=512, kd=256)


def test_a_sampling_group_on_an_fp8_backend_without_the_fp8_sampling_head_is_refused():
    with pytest.raises(ValueError, match="decb_lm_head_sample_fp8"):
        StreamGroup(_fake_engine(RecordingOps(without=("decb_lm_head_sample_fp8",)), True), 2, sampling=True)
    # the greedy entries are asked for first, as without sampling
    with pytest.raises(ValueError, match="llm_fp8"):
        StreamGroup(_fake_engine(RecordingOps(without=FP8_GROUP_OPS), True), 2, sampling=True)


@pytest.mark.parametrize("fp8", [False, True])
def test_a_sampled_step_ends_in_the_sampling_pair_and_a_greedy_step_in_the_greedy_pair(fp8):
    ops = RecordingOps()
    group = StreamGroup.__new__(StreamGroup)
    group.engine = _fake_engine(ops, fp8)
    group.table, group.samples, group.x, group.q, group.attn, group.h, group.logits, group.ws, group.suppress = \
        "tab", "smp", "x", ["q0", "q1"], ["a0", "a1"], "h", "logits", "ws", "sup"
    lane = SimpleNamespace(rope_cs="rope", d_ws="dws", _attn_len=64, decode_chunk=32, state=[0, 0])
    act = [(lane, SimpleNamespace(pool="pool", slot_of_dev="slots"))] * 2
    sfx = "_fp8" if fp8 else ""
    group._step_launch(act, True)
    names = [c[0] for c in ops.calls]
    assert names[-2:] == ["decb_lm_head_sample" + sfx, "decb_sample_finish"] and "decb_argmax_finish" not in names
    head, fin = ops.calls[-2][1], ops.calls[-1][1]
    assert head[:3] == ("tab", "smp", 2) and head[3:5] == ("x", "final_norm") and head[-3:] == ("logits", "sup", "ws")
    assert (head[6:8] == ("lm_head8", "lm_head_s")) if fp8 else (head[6] == "lm_head")
    assert fin == ("tab", "smp", 2, "logits", "sup", "ws", 1000, 1)
    layers = names[:-2]
    ops.calls.clear()
    group._step_launch(act, False)
    names = [c[0] for c in ops.calls]
    assert names[-2:] == ["decb_lm_head" + sfx, "decb_argmax_finish"] and names[:-2] == layers, "the layers do not depend on the token choice"
