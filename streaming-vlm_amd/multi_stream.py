"""Parallelism across streams.  Across GPUs: one independent process per GPU (reference:
eval/livesports3kcc/distributed_generate_streaming.py:55,62,127-143: N processes, `cuda:{rank}`, strided
sample sharding, results joined outside the model; no data-path communication).  On one GPU: a stream group
(`streaming_inference_group`, stream_group.py): up to 4 streams share one weight set and decode in lock-step.

`torch.distributed` ("nccl" == RCCL over xGMI on ROCm, "gloo" in CPU tests) is used for exactly two things,
both OUTSIDE the timed region: a barrier on each side of it and one all_gather of three doubles per rank.
"""
from __future__ import annotations

import os
from typing import List, Optional

import torch


def env_rank():
    return int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("LOCAL_RANK", "0"))


def init_distributed(backend: Optional[str] = None):
    """Returns (dist or None, rank, world, local_rank).  Rendezvous comes from MASTER_ADDR/MASTER_PORT."""
    rank, world, local_rank = env_rank()
    if world == 1:
        return None, 0, 1, local_rank
    import torch.distributed as dist
    if backend is None:
        backend = "nccl" if torch.cuda.is_available() else "gloo"
    kw = {}
    if backend == "nccl":
        torch.cuda.set_device(local_rank)
        kw["device_id"] = torch.device("cuda", local_rank)
    dist.init_process_group(backend=backend, rank=rank, world_size=world, **kw)
    return dist, rank, world, local_rank


def shard(items: List, rank: int, world: int) -> List:
    """Strided sharding of independent units (streams / samples): item i -> rank i mod world."""
    return items[rank::world]


def fence(dist, device=None):
    """barrier bracketed by device syncs: everything enqueued before is finished on every rank."""
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    if torch.cuda.is_available():
        torch.cuda.synchronize()


def aggregate(frames: float, tokens: float, seconds: float, dist, device="cpu") -> dict:
    """Whole-job throughput = units of ALL ranks / slowest rank's time."""
    mine = torch.tensor([frames, tokens, seconds], dtype=torch.float64, device=device)
    if dist is None:
        allst = mine.cpu().unsqueeze(0)
    else:
        parts = [torch.zeros_like(mine) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, mine)
        allst = torch.stack(parts).cpu()
    t_max = float(allst[:, 2].max())
    return {"frames_per_sec": float(allst[:, 0].sum()) / t_max, "tokens_per_sec": float(allst[:, 1].sum()) / t_max,
            "t_max": t_max, "per_rank_frames_per_sec": (allst[:, 0] / allst[:, 2]).tolist(), "world": allst.shape[0]}


# ----------------------------------------------------------------------------- several streams on one GPU
class StreamGroupError(RuntimeError):
    """A stream of `streaming_inference_group` raised: `.index` is its position in `streams`, `.results` the per-stream response
    lists of the streams that completed (None for those that did not); the stream's own exception is the `__cause__`."""

    def __init__(self, index: int, results: List, cause: BaseException):
        super().__init__(f"stream {index} failed: {type(cause).__name__}: {cause}")
        self.index, self.results = index, results


def streaming_inference_group(model, processor, streams: List[dict], n_lanes: Optional[int] = None, group=None, sampling: bool = False,
                              wide: bool = False, batched_attn: bool = False, **common_kw) -> List:
    """Run `len(streams)` streams on ONE GPU through a stream group: each entry of `streams` holds the per-stream keyword arguments of
    `streaming_inference` (video_path, query, previous_text, duration, ...), `common_kw` the shared ones.  Every stream runs the
    unchanged `streaming_inference` loop in its own host thread against its lane's model object; the lanes' generate() calls meet in
    the group, which runs one batch when every lane that still has a stream has a request pending.  `n_lanes` defaults to min(3, streams): the measured
    aggregate throughput stops growing there.  More streams than lanes: they are
    queued, and a lane that finishes a stream takes the next one; a lane with nothing left detaches and the rest carry on.
    Token choice: greedy only by default (pass do_sample=False, or top_k=1); with `sampling=True` the group is built as
    `StreamGroup(..., sampling=True)` and every stream may carry its own `do_sample / temperature / top_k / top_p / generator` -- each
    lane then produces the tokens of that stream run alone on a fresh model with the same generator seed (an existing `group` passed in
    keeps the setting it was built with).  `wide=True` builds `StreamGroup(..., wide=True)`: up to 16 lanes on the MFMA decode kernels
    (bf16 weights, greedy; `n_lanes` still defaults to min(3, streams)).  `batched_attn=True` builds `StreamGroup(..., batched_attn=True)`:
    the decode attention of all lanes in one launch pair per layer (same tokens; combines with every other option).  Strict-causal (no look-ahead ViT).  Returns the per-stream response
    lists in the order of `streams`; if a stream raised, the others still run to their end and a `StreamGroupError` naming the first
    failed stream's index is raised afterwards."""
    import threading
    from .driver import streaming_inference
    from .stream_group import DEFAULT_LANES, StreamGroup
    if group is None:
        # an option that is off is not passed: stand-ins for StreamGroup that older tests substitute do not know the keyword
        opt = {"batched_attn": True} if batched_attn else {}
        group = StreamGroup(model._svlm_engine, min(DEFAULT_LANES, len(streams)) if n_lanes is None else n_lanes, sampling=sampling,
                            wide=wide, **opt)
    results: List = [None] * len(streams)
    errors = {}
    lock = threading.Lock()
    todo = list(range(len(streams)))

    def lane_thread(i):
        lane_model = group.lane_model(i)
        try:
            while True:
                with lock:
                    if not todo:
                        return
                    s = todo.pop(0)
                try:
                    results[s] = streaming_inference(model=lane_model, processor=processor, **{**common_kw, **streams[s]})
                except BaseException as e:          # this stream only: the lane goes on to the next one
                    errors[s] = e
        finally:
            group.detach(i)

    n = min(group.n_lanes, len(streams))
    for i in range(n):
        group.attach(i)                              # all lanes are attached before any of them can complete a batch alone
    threads = [threading.Thread(target=lane_thread, args=(i,), name=f"svlm-lane-{i}", daemon=True) for i in range(n)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        first = min(errors)
        raise StreamGroupError(first, results, errors[first]) from errors[first]
    return results


# ----------------------------------------------------------------------------- sample-sharded generation
def streaming_worker(rank: int, world: int, records: List[dict], model, processor, save_dir: str, simple_ctx: bool = False,
                     repetition_penalty: float = 1.05, temperature: float = 0.9, **stream_kw) -> List[int]:
    """One rank of the reference's LiveSports-3K-CC generation (eval/livesports3kcc/distributed_generate_streaming.py:44-121):
    record i goes to rank i mod world (:62), every finished record is one `{save_dir}/{i}.json` (resumable, :69-71), prompts are
    built as at :87-96.  `records` replaces the `datasets` download (needs network): dicts with video, video_id, event_id,
    begin, end, event_title, preasr_text.  Returns the indices this rank produced."""
    import json
    from .driver import streaming_inference
    os.makedirs(save_dir, exist_ok=True)
    done = []
    for idx in shard(list(range(len(records))), rank, world):
        save_path = os.path.join(save_dir, f"{idx}.json")
        if os.path.exists(save_path):
            continue
        r = records[idx]
        title, preasr = r.get("event_title"), r.get("preasr_text")
        if simple_ctx:
            title = "" if preasr else title
            prompt = f"{title}\n{preasr}".strip()
        else:
            prompt = ("You are an expert video commentator providing real-time, insightful, and engaging commentary on visual content.\n")
            if title:
                prompt += f"This is a video titled \"{title}\".\n"
        responses = streaming_inference(model=model, processor=processor, query=prompt, previous_text=preasr if preasr else "",
                                        video_path=r["video"], skip_first_chunk=r["begin"], duration=r["end"] - r["begin"],
                                        temperature=temperature, repetition_penalty=repetition_penalty, quiet=True, **stream_kw)
        with open(save_path, "w") as wf:
            json.dump({"video_id": r.get("video_id"), "event_id": r.get("event_id"), "begin": r["begin"], "end": r["end"],
                       "pred": "".join(x["response"] for x in responses)}, wf)
        done.append(idx)
    return done


def join_jsonl(save_dir: str) -> str:
    """jsons -> jsonl, as the reference does after its workers finish (:138-150)."""
    import json
    out = save_dir.rstrip("/") + ".jsonl"
    with open(out, "w") as wf:
        for name in sorted(os.listdir(save_dir), key=lambda n: int(n.split(".")[0]) if n.split(".")[0].isdigit() else 1 << 30):
            try:
                wf.write(json.dumps(json.load(open(os.path.join(save_dir, name)))) + "\n")
            except Exception:
                continue
    return out
