"""Every sampled token, predicted exactly: svlm_penalty_sample and the fused lm_head candidates replayed draw by draw against the
float64 reference of tests/sampling_ref64.py (Philox is counter-based, so a token is a function of seed, step, logits, seen, suppress).
A decided draw -- farther from its decision boundary than the kernels' fp32 arithmetic can move it, by the bounds derived in that
module -- must equal the kernel's token; the case list (tests/sampling_cases.py) caps the undecided ones at 1 % per case."""
import numpy as np
import pytest
import torch

import sampling_cases as SC
import sampling_ref64 as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
SENTINEL = -77
TAIL = 4                     # sentinel entries behind the last draw


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def _i32(seq):
    return torch.tensor([int(np.int32(np.uint32(int(v) & 0xFFFFFFFF))) for v in seq], dtype=torch.int32)


def report(name, case, row, seen0, toks, ref):
    """Print draws / undecided / mismatches, and for the first mismatch what is needed to read it without another run."""
    dec = ref["decided"]
    bad = np.nonzero(dec & (ref["tokens"] != toks))[0]
    print(f"[replay {name}] mode={R.MODE_NAMES[ref['mode']]} draws={toks.size} undecided={int((~dec).sum())} mismatches={bad.size}")
    if bad.size:
        i = int(bad[0])
        d = R.replay(case, row, seen0, gpu_tokens=toks, detail_at=i)["detail"]
        print(f"  first mismatch at draw {i} (step {case['state'][1] + 1 + i}): expected {d['token']} (p={d['prob'](d['token']):.3e}), "
              f"got {int(toks[i])} (p={d['prob'](int(toks[i])):.3e}); nearest decision boundary {d['dist']:.3g} bounds away; "
              f"survivor margin {d['margin']:.3g}")
    return bad.size


def run_penalty_sample(ops, case, logits, seen0):
    n, start = case["n_draws"], case["state"][1] + 1
    d_logits = torch.from_numpy(logits).cuda()
    d_seen = None if seen0 is None else torch.from_numpy(seen0).cuda()
    d_sup = _i32(case["suppress"]).cuda() if case["suppress"] else None
    tok_buf = torch.full((start + n + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    state = torch.tensor(list(case["state"]), dtype=torch.int32, device="cuda")
    rng = _i32(case["seed"]).cuda()
    ws = ops.sampling_ws(case["V"], "cuda")
    for _ in range(n):
        ops.penalty_sample(d_logits, d_seen, case["penalty"], d_sup, case["T"], case["top_k"], case["top_p"], rng, tok_buf, state,
                           case["advance_kv"], ws)
    torch.cuda.synchronize()
    return tok_buf.cpu().numpy(), state.cpu().tolist(), None if d_seen is None else d_seen.cpu().numpy()


def check_run(name, case, row, seen0, buf, state, seen, ref):
    n, start = case["n_draws"], case["state"][1] + 1
    assert (buf[:start] == SENTINEL).all() and (buf[start + n:] == SENTINEL).all(), f"{name}: tok_buf written outside the {n} draws"
    assert state == ref["state"], (name, state, ref["state"])
    if seen0 is not None:
        assert np.array_equal(seen, ref["seen"]), f"{name}: `seen` differs from the replay at {np.nonzero(seen != ref['seen'])[0][:8]}"
    toks = buf[start:start + n]
    assert ((toks >= 0) & (toks < case["V"])).all(), f"{name}: token out of range"
    assert report(name, case, row, seen0, toks, ref) == 0, f"{name}: a decided draw differs from the kernel's token"
    assert (~ref["decided"]).sum() <= R.UNDECIDED_CAP * n, f"{name}: undecided draws above the cap"


def check_drawn_set(case, toks, ref):
    """check = set: the drawn set is the survivor set (every survivor that 2000 draws cannot miss: P(never) < 1e-12); peak: one token."""
    drawn = set(int(t) for t in toks)
    surv = set(np.nonzero(ref["survivors"])[0].tolist()) if ref["survivors"] is not None else None
    if surv is not None:
        assert drawn <= surv, f"{case['name']}: drawn outside the survivor set: {sorted(drawn - surv)[:8]}"
    if case["check"] in ("set", "zeros"):
        certain = SC.certain_survivors(case)
        assert certain <= drawn, f"{case['name']}: survivors never drawn: {sorted(certain - drawn)}"
    if case["check"] == "peak":
        assert drawn == {case["V"] // 3}, drawn


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["name"])
def test_penalty_sample_replays_exactly(ops, case):
    logits, seen0 = SC.materialise(case)
    buf, state, seen = run_penalty_sample(ops, case, logits, seen0)
    start, n = case["state"][1] + 1, case["n_draws"]
    toks = buf[start:start + n].astype(np.int64)
    ref = R.replay(case, logits, seen0, gpu_tokens=np.clip(toks, 0, case["V"] - 1))
    check_run(case["name"], case, logits, seen0, buf, state, seen, ref)
    check_drawn_set(case, toks, ref)
    buf2, state2, seen2 = run_penalty_sample(ops, case, logits, seen0)          # the order the atomics land in must not matter
    assert np.array_equal(buf2, buf) and state2 == state, f"{case['name']}: a second run from the same buffers drew other tokens"
    assert seen0 is None or np.array_equal(seen2, seen)


# ------------------------------------------------------------------------------------------------ the fused head
HEADS = [("bf16", 130, 256, False), ("bf16", 4096, 256, False), ("bf16", 3001, 1544, False), ("bf16", 130, 256, True),
         ("fp8", 130, 256, False), ("fp8", 4096, 256, False)]
STEPS = 500


def _head(ops, family, V, K, pad):
    import gemv_paths as G
    if family == "fp8" and not hasattr(ops.lib, "svlm_dec_lm_head_sample_fp8"):
        return None
    o = G.weights(family, "iid", V, K, seed=V + K, device="cuda")
    x, gain = [t.cuda() for t in G.activation_row("iid", K, True, seed=V)]
    if family == "bf16":
        W = G.pad_rows("bf16", o) if pad else o["W"]
        assert W.is_cuda and W.stride(0) == (K + 8 if pad else K)
        return (lambda *a, **kw: ops.dec_lm_head(x, gain, 1e-6, W, *a, **kw)), (W,)
    W8, s8 = o["W8"], o["s8"]
    return (lambda *a, **kw: ops.dec_lm_head_fp8(x, gain, 1e-6, W8, s8, *a, **kw)), (W8.view(torch.uint8), s8)


@pytest.mark.parametrize("family,V,K,pad", HEADS, ids=lambda v: str(v))
def test_fused_head_sample_replays_exactly(ops, family, V, K, pad):
    """svlm_dec_lm_head_sample[_fp8] + svlm_argmax_finish, 500 steps with live `seen`: the token is the reference's Gumbel argmax over
    the kernel's own fp32 logits row (which tests/test_gemv_paths_gpu.py holds to fp64)."""
    head = _head(ops, family, V, K, pad)
    if head is None:
        return                                         # a backend without the e4m3 twin has nothing to replay
    lm_head, _ = head
    case = dict(name=f"head-{family}-V{V}-K{K}{'-pad' if pad else ''}", V=V, top_k=0, top_p=1.0, T=0.8, penalty=1.05, suppress=None,
                seed=(2024, 0x9E3779B9), state=(31, 6), advance_kv=1, n_draws=STEPS, check=None)
    g = torch.Generator().manual_seed(V)
    seen0 = (torch.rand(V, generator=g) < 0.2).to(torch.uint8).numpy()
    logits = torch.zeros(V, dtype=torch.float32, device="cuda")
    ws = ops.sampling_ws(V, "cuda")
    lm_head(logits, None, 1.0, None, ws)                                         # the row itself, to pick the suppressed ids from
    ops.argmax_finish(ws, V, None, torch.zeros(2, dtype=torch.int32, device="cuda"), torch.tensor([0, -1], dtype=torch.int32, device="cuda"), 0)
    row0 = logits.cpu().numpy().copy()
    top = np.argsort(-row0, kind="stable")
    case["suppress"] = (int(top[0]), int(top[3]))                                 # the raw argmax and one more of the largest
    seen0[top[3]] = 1
    start = case["state"][1] + 1
    d_seen, d_sup = torch.from_numpy(seen0.copy()).cuda(), _i32(case["suppress"]).cuda()
    tok_buf = torch.full((start + STEPS + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
    state = torch.tensor(list(case["state"]), dtype=torch.int32, device="cuda")
    rng = _i32(case["seed"]).cuda()
    rows = torch.empty((STEPS, V), dtype=torch.float32, device="cuda")
    for i in range(STEPS):
        lm_head(logits, d_seen, case["penalty"], d_sup, ws, temperature=case["T"], rng=rng, state=state)
        ops.argmax_finish(ws, V, d_seen, tok_buf, state, case["advance_kv"])
        rows[i].copy_(logits)
    torch.cuda.synchronize()
    assert bool((rows == rows[0]).all()) and np.array_equal(rows[0].cpu().numpy(), row0), "the logits row moved between steps"
    buf = tok_buf.cpu().numpy()
    toks = buf[start:start + STEPS].astype(np.int64)
    ref = R.replay(case, row0, seen0, gpu_tokens=np.clip(toks, 0, V - 1))
    check_run(case["name"], case, row0, seen0, buf, state.cpu().tolist(), d_seen.cpu().numpy(), ref)
    assert not set(toks.tolist()) & set(case["suppress"])


@pytest.mark.parametrize("family,V,K,pad", HEADS, ids=lambda v: str(v))
def test_fused_head_greedy_is_the_exact_argmax(ops, family, V, K, pad):
    """svlm_dec_lm_head[_fp8] (no rng) + svlm_argmax_finish: the argmax of the processed row, the lowest index among equal scores --
    two identical weight rows that hold the maximum."""
    head = _head(ops, family, V, K, pad)
    if head is None:
        return
    lm_head, W = head
    logits = torch.zeros(V, dtype=torch.float32, device="cuda")
    ws = ops.sampling_ws(V, "cuda")
    g = torch.Generator().manual_seed(V + 1)
    seen0 = (torch.rand(V, generator=g) < 0.2).to(torch.uint8).numpy()

    def step(seen, sup):
        tok_buf = torch.full((1 + TAIL,), SENTINEL, dtype=torch.int32, device="cuda")
        state = torch.tensor([5, -1], dtype=torch.int32, device="cuda")
        d_seen = None if seen is None else torch.from_numpy(seen.copy()).cuda()
        lm_head(logits, d_seen, 1.05, None if sup is None else _i32(sup).cuda(), ws)
        ops.argmax_finish(ws, V, d_seen, tok_buf, state, 1)
        torch.cuda.synchronize()
        buf = tok_buf.cpu().numpy()
        assert (buf[1:] == SENTINEL).all() and state.cpu().tolist() == [6, 0]
        row = logits.cpu().numpy().copy()
        want = R.expected(R.GREEDY, R.processed(row, seen, 1.05, sup, np.float32(1.0)), 1, 1.0, None, 0)["token"]
        assert int(buf[0]) == want, (int(buf[0]), want)
        if seen is not None:
            seen[want] = 1
            assert np.array_equal(d_seen.cpu().numpy(), seen)
        return row, want

    row, a = step(None, None)
    b = a - 3 if a >= 3 else a + 3                       # a second row with the same weights (and the same e4m3 row scale)
    for t in W:
        t[b].copy_(t[a])
    row, t = step(None, None)
    assert row[a] == row[b] == row.max() and t == min(a, b), (a, b, t, row[a], row[b])
    step(seen0.copy(), None)
    step(seen0.copy(), (min(a, b), int(np.argsort(-row)[4])))    # the lower twin suppressed: the higher one wins (unless penalised away)


# ------------------------------------------------------------------------------------------------ argument checks
def test_bad_sampling_arguments_are_refused_and_change_nothing(ops):
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import _ptr, _stream
    V = 130
    logits = torch.randn(V, generator=torch.Generator().manual_seed(0)).cuda()
    tok_buf = torch.full((8,), SENTINEL, dtype=torch.int32, device="cuda")
    state = torch.tensor([3, 1], dtype=torch.int32, device="cuda")
    rng, ws = _i32((1, 2)).cuda(), ops.sampling_ws(V, "cuda")
    sup9 = torch.arange(9, dtype=torch.int32, device="cuda")
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(suppress=sup9)]
    for kw in bad:
        a = dict(temperature=0.9, top_k=50, top_p=0.9, suppress=None)
        a.update(kw)
        with pytest.raises(_lib.SvlmError):
            ops.penalty_sample(logits, None, 1.0, a["suppress"], a["temperature"], a["top_k"], a["top_p"], rng, tok_buf, state, 1, ws)
    with pytest.raises(_lib.SvlmError):                  # missing rng: straight at the C entry (the wrapper dereferences it first)
        ops._check(ops.lib.svlm_penalty_sample(_ptr(logits), V, 0, 1.0, 0, 0, 0.9, 50, 0.9, 0, _ptr(tok_buf), _ptr(state), 1, _ptr(ws), _stream()),
                   "svlm_penalty_sample")
    torch.cuda.synchronize()
    assert (tok_buf.cpu() == SENTINEL).all() and state.cpu().tolist() == [3, 1]
