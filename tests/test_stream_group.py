"""The host side of stream groups without a GPU: the lanes' rendezvous against a stub that records the batches, the multi-stream driver
on top of it, the refused options, and the ABI of the lane-batched kernels.  Every wait has a timeout: a bug fails, it does not hang."""
import ctypes
import os
import re
import threading

import pytest

from streaming_vlm_amd.stream_group import LaneRendezvous, StreamGroup, check_request

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAIT = 10.0


class Recorder:
    """run_batch stub: notes which lanes were in each batch; a request {'raise': exc} makes that lane's result the exception."""

    def __init__(self):
        self.batches = []

    def __call__(self, requests):
        self.batches.append(tuple(i for i, r in enumerate(requests) if r is not None))
        return [None if r is None else (r["raise"] if "raise" in r else ("done", i, r["chunk"])) for i, r in enumerate(requests)]


def _spawn(fn, *args):
    box = {}

    def run():
        try:
            box["out"] = fn(*args)
        except BaseException as e:
            box["err"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start()
    return t, box


def _join(t):
    t.join(WAIT)
    assert not t.is_alive(), "a lane thread is stuck in the rendezvous"


def test_batch_fires_only_when_every_attached_lane_is_pending():
    rec = Recorder()
    rv = LaneRendezvous(3, rec)
    for i in range(3):
        rv.attach(i)
    t0, b0 = _spawn(rv.submit, 0, dict(chunk=0), WAIT)
    t1, b1 = _spawn(rv.submit, 1, dict(chunk=0), WAIT)
    t0.join(0.3)
    assert t0.is_alive() and t1.is_alive() and rec.batches == [], "two of three lanes pending: no batch yet"
    t2, b2 = _spawn(rv.submit, 2, dict(chunk=0), WAIT)
    for t in (t0, t1, t2):
        _join(t)
    assert rec.batches == [(0, 1, 2)]
    assert [b["out"] for b in (b0, b1, b2)] == [("done", i, 0) for i in range(3)]


def test_detach_shrinks_the_batch_and_wakes_the_waiters():
    rec = Recorder()
    rv = LaneRendezvous(3, rec)
    for i in range(3):
        rv.attach(i)
    t0, b0 = _spawn(rv.submit, 0, dict(chunk=1), WAIT)
    t2, b2 = _spawn(rv.submit, 2, dict(chunk=1), WAIT)
    t0.join(0.3)
    assert rec.batches == []
    rv.detach(1)                                  # lane 1's stream has ended: the two that wait make the batch
    _join(t0); _join(t2)
    assert rec.batches == [(0, 2)] and b0["out"] == ("done", 0, 1) and b2["out"] == ("done", 2, 1)
    rv.detach(2)
    assert rv.submit(0, dict(chunk=2), WAIT) == ("done", 0, 2) and rec.batches[-1] == (0,)
    with pytest.raises(RuntimeError):
        rv.submit(1, dict(chunk=0), WAIT)         # not attached


def test_an_exception_reaches_its_own_lane_only():
    rec = Recorder()
    rv = LaneRendezvous(2, rec)
    rv.attach(0); rv.attach(1)
    t0, b0 = _spawn(rv.submit, 0, {"chunk": 0, "raise": KeyError("lane 0 broke")}, WAIT)
    t1, b1 = _spawn(rv.submit, 1, dict(chunk=0), WAIT)
    _join(t0); _join(t1)
    assert isinstance(b0.get("err"), KeyError) and b1.get("out") == ("done", 1, 0)
    # a batch that fails as a whole is heard by every lane of it, and the rendezvous stays usable
    boom = LaneRendezvous(2, lambda reqs: (_ for _ in ()).throw(OSError("device lost")))
    boom.attach(0); boom.attach(1)
    ta, ba = _spawn(boom.submit, 0, {}, WAIT)
    tb, bb = _spawn(boom.submit, 1, {}, WAIT)
    _join(ta); _join(tb)
    assert isinstance(ba.get("err"), OSError) and isinstance(bb.get("err"), OSError)


def test_a_lane_that_never_gets_its_batch_times_out():
    rv = LaneRendezvous(2, Recorder())
    rv.attach(0); rv.attach(1)
    with pytest.raises(TimeoutError):
        rv.submit(0, dict(chunk=0), 0.2)


class StubGroup:
    """What streaming_inference_group needs of a group, over a recording run_batch."""

    def __init__(self, n_lanes, rec):
        self.n_lanes = n_lanes
        self._rv = LaneRendezvous(n_lanes, rec)
        self.attach, self.detach, self.submit = self._rv.attach, self._rv.detach, self._rv.submit

    def lane_model(self, i):
        return (self, i)


def test_queued_streams_take_freed_lanes_and_a_failing_stream_is_reported_with_its_index(monkeypatch):
    from streaming_vlm_amd import driver, multi_stream
    rec = Recorder()
    group = StubGroup(2, rec)

    def fake_streaming_inference(model=None, processor=None, name=None, chunks=0, fail_at=None, **kw):
        grp, lane = model
        out = []
        for c in range(chunks):
            if fail_at == c:
                raise ValueError(f"{name} broke at chunk {c}")
            out.append(dict(response=f"{name}:{grp.submit(lane, dict(chunk=c), WAIT)[2]}"))
        return out

    monkeypatch.setattr(driver, "streaming_inference", fake_streaming_inference)
    streams = [dict(name="a", chunks=3), dict(name="b", chunks=1), dict(name="c", chunks=2), dict(name="d", chunks=4)]
    box = {}
    t = threading.Thread(target=lambda: box.update(out=multi_stream.streaming_inference_group(None, None, streams, group=group)), daemon=True)
    t.start(); _join(t)
    assert [[r["response"] for r in s] for s in box["out"]] == [[f"{s['name']}:{c}" for c in range(s["chunks"])] for s in streams]
    assert all(len(b) in (1, 2) for b in rec.batches) and sum(len(b) for b in rec.batches) == 10
    assert rec.batches[0] == (0, 1), "both lanes attached before the first batch"
    # stream 1 raises in its second chunk: the caller hears its index after the others have completed
    streams[1] = dict(name="b", chunks=3, fail_at=1)
    group = StubGroup(2, Recorder())
    box = {}

    def run():
        try:
            multi_stream.streaming_inference_group(None, None, streams, group=group)
        except multi_stream.StreamGroupError as e:
            box["err"] = e
    t = threading.Thread(target=run, daemon=True)
    t.start(); _join(t)
    err = box["err"]
    assert err.index == 1 and isinstance(err.__cause__, ValueError) and err.results[1] is None
    assert [len(r) for i, r in enumerate(err.results) if i != 1] == [3, 2, 4]


def test_refused_options_raise_the_documented_errors():
    ok = dict(ids=[1, 2], cache=None, video_grid_thw=[], max_new_tokens=4)
    assert "next_vision" not in check_request(dict(ok, next_vision=(object(), [[1, 2, 2]])))        # declined, not an error
    assert check_request(dict(ok, do_sample=True, top_k=1))["top_k"] == 1
    for bad in (dict(do_sample=True), dict(do_sample=True, top_k=50), dict(do_sample=True, top_k=0, top_p=0.9), dict(force_tokens=[3]),
                dict(keep_logits=True)):
        with pytest.raises(ValueError, match="stream group"):
            check_request(dict(ok, **bad))

    class Eng:
        llm_fp8, decode_tail = False, False
    with pytest.raises(ValueError, match="n_lanes"):
        StreamGroup(Eng(), 0)
    with pytest.raises(ValueError, match="n_lanes"):
        StreamGroup(Eng(), 5)
    fp8 = Eng(); fp8.llm_fp8 = True
    with pytest.raises(ValueError, match="llm_fp8"):
        StreamGroup(fp8, 2)
    tail = Eng(); tail.decode_tail = True
    with pytest.raises(ValueError, match="decode_tail"):
        StreamGroup(tail, 2)


def test_lane_record_layout_and_batched_entry_points_are_declared_exported_and_bound():
    """Header, ctypes table and library agree on the lane-batched entries; the host-side record has the header's 72-byte layout."""
    import sys
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import HipOps
    names = ["svlm_decb_embed", "svlm_decb_qkv", "svlm_decb_gemv", "svlm_decb_gate_up", "svlm_decb_lm_head", "svlm_decb_lm_head_ws_stride",
             "svlm_decb_argmax_finish"]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "svlm.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(ROOT, "streaming-vlm_amd", "libsvlm_hip.so"))
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr) and n in _lib.SIGNATURES and getattr(lib, n)
        n_args = len([a for a in re.search(r"\b%s\s*\(([^)]*)\)" % n, hdr).group(1).split(",") if a.strip()])
        assert n_args == len(_lib.SIGNATURES[n][1]), n
    assert "typedef struct svlm_lane" in hdr and HipOps.LANE_WORDS * 8 == 72
    fields = re.search(r"typedef struct svlm_lane \{(.*?)\} svlm_lane;", hdr, flags=re.S).group(1)
    sizes = [8 if "*" in f else 4 for f in fields.split(";") if f.strip()]
    assert sum(sizes) == 72 and sizes[:6] == [8] * 6
    # candidates of a lane: 8 bytes per workgroup of 8 vocabulary rows, rounded to 16 (host arithmetic)
    assert _lib.load().svlm_decb_lm_head_ws_stride(151936) == 151936 and _lib.load().svlm_decb_lm_head_ws_stride(20) == 32
    assert _lib.load().svlm_decb_lm_head_ws_stride(0) < 0
