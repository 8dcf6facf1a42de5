"""bench.py --dump-outputs: what the helpers capture is what the path handed its caller for that chunk (tokens, the last
forward's logits, rows of past_key_values), written as float32 / float64 .npy.  Runs the tiny model on the CPU test backend."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _stream(n_chunks, capture_at):
    import bench
    import streaming_vlm_amd as S
    from streaming_vlm_amd import config as C
    from streaming_vlm_amd.weights import random_state_dict
    from ref_ops import RefOps
    cfg = C.tiny()
    model = S.StreamingQwen2VL(cfg, random_state_dict(cfg, 0, "cpu"), "cpu", ops=RefOps(), max_len=512, max_new_tokens=4, use_graph=False)
    log, counts, got = [], [], {}

    def cb(i):
        if i == capture_at:
            eng = model._svlm_engine
            got.update(bench.capture_outputs(eng, counts[-1]))
            got["_kv"] = [tuple(t[0].float().numpy() for t in eng._last_cache.layer_kv(l)) for l in range(cfg.text.num_layers)]
    S.streaming_inference(model=model, processor=S.SyntheticProcessor(), video_path="synthetic://56x56@1fps?stream=0", model_base="Qwen2",
                          duration=n_chunks, kv_policy="sink_window", sink=4, window=64, do_sample=False, max_new_tokens=4,
                          suppress_eos=True, quiet=True, ids_log=log, token_counts=counts, keep_logits=True, chunk_callback=cb)
    return got, log, counts


def test_captured_outputs_are_the_chunk_results(tmp_path):
    import bench
    got, log, counts = _stream(4, 3)                 # captured between chunk 2 and chunk 3: chunk 2's results
    kv = got.pop("_kv")
    n = counts[2]
    assert got["tokens"].dtype == np.float64 and got["tokens"].tolist() == log[2]["new"][:n]
    assert got["logits"].dtype == np.float32 and np.array_equal(got["logits"], log[2]["logits"][-1].numpy())
    L = int(got["kv_len"][0])
    assert L == log[2]["kv_len"]
    rows = got["kv_sample_rows"].astype(np.int64)
    assert rows.min() >= 0 and rows.max() == L - 1 and len(np.unique(rows)) == len(rows)
    assert set(range(L - bench.KV_TAIL_ROWS, L)) <= set(rows.tolist()) and len(rows) <= bench.KV_SAMPLE_ROWS + bench.KV_TAIL_ROWS
    ks = got["kv_sample"]
    assert ks.dtype == np.float32 and ks.shape == (len(kv), 2, kv[0][0].shape[0], len(rows), kv[0][0].shape[2])
    for layer, (k, v) in enumerate(kv):                # the sample is past_key_values' (1, Hkv, L, D) views at those rows
        assert np.array_equal(ks[layer, 0], k[:, rows]) and np.array_equal(ks[layer, 1], v[:, rows])

    shapes = bench.dump_outputs(str(tmp_path / "d"), got)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f"{k}.npy" for k in got)
    for name, a in got.items():
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype in (np.float32, np.float64) and list(b.shape) == shapes[name] and np.array_equal(a, b)


def test_same_arguments_same_outputs():
    a, _, _ = _stream(3, 2)
    b, _, _ = _stream(3, 2)
    for name in ("tokens", "logits", "kv_sample", "kv_sample_rows", "kv_len"):
        assert np.array_equal(a[name], b[name]), name


def test_dump_refuses_more_than_the_limit(tmp_path):
    import bench
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path), {"big": np.zeros(bench.DUMP_LIMIT_BYTES // 8 + 1, dtype=np.float64)})


def test_cli_has_full_and_dump_outputs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=120)
    assert bad.returncode != 0 and "--steps" in bad.stderr
