"""CPU checks of the exact sampling replay machinery (no GPU): the Philox mirror against known answers and the literals of
csrc/common.h; the float64 survivor rule against the oracle's restatement of HF's warpers; the cap, margin and coverage conditions of
the case list; an fp32 emulation of the two kernel bodies' arithmetic that must agree with the reference on every decided draw; and
faults injected into that emulation, each of which the reference must catch."""
import os
import re

import numpy as np
import pytest
import torch

import sampling_cases as SC
import sampling_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "streaming-vlm_amd", "csrc")
F32 = np.float32
SMALL = [c for c in SC.CASES if c["V"] <= 3001]


# ------------------------------------------------------------------------------------------------ Philox and the constants
@pytest.mark.parametrize("ctr,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1")])
def test_philox_known_answers(ctr, key, want):
    assert " ".join("%08x" % int(w) for w in R.philox4(*ctr, *key)) == want
    vec = R.philox4(np.array([ctr[0], 1, 2]), ctr[1], ctr[2], ctr[3], *key)          # vectorised over c0: lane 0 is the scalar answer
    assert "%08x" % int(vec[0][0]) == want[:8] and len(set(int(x) for x in vec[0])) == 3
    if ctr[2] == 0 and ctr[3] == 0:
        assert int(R.philox_first(ctr[0], ctr[1], *key)) == int(want[:8], 16)


def test_constants_are_the_literals_of_common_h():
    src = open(os.path.join(CSRC, "common.h")).read()
    body = src[src.index("svlm_philox_first"):src.index("svlm_env")]
    hexes = [int(h, 16) for h in re.findall(r"0x([0-9A-Fa-f]{8})u", body)]
    assert hexes == [R.PHILOX_M0, R.PHILOX_M1, R.PHILOX_W0, R.PHILOX_W1], [hex(h) for h in hexes]
    assert "for (int r = 0; r < 10; ++r)" in body and "unsigned c2 = 0u, c3 = 0u;" in body
    uni = re.search(r"svlm_philox_first\(idx, step, rng\[0\], rng\[1\]\) >> (\d+)\) \+ 0\.5f\) \* \(1\.0f / ([0-9.]+)f\)", body)
    assert int(uni.group(1)) == R.UNIFORM_SHIFT and 1.0 / float(uni.group(2)) == R.UNIFORM_SCALE
    gum = re.search(r"\(\(float\)svlm_philox_first\(idx, step, rng\[0\], rng\[1\]\) \+ 0\.5f\) \* \(1\.0f / ([0-9.]+)f\)", body)
    assert 1.0 / float(gum.group(1)) == R.GUMBEL_SCALE and "return -logf(-log1pf(-v));" in body
    smp = open(os.path.join(CSRC, "dec_sample.h")).read()
    assert "svlm_philox_uniform(rng, (unsigned)(state[1] + 1), 0xFFFFFFFFu)" in smp and "#define SF_CAP 2048" in smp
    assert "__float_as_uint(x + 0.0f)" in smp, "sf_key canonicalises the zero"
    assert 0 < float(R.uniform((1, 2), 3)) < 1


def test_sample_mode_is_the_dispatch_of_the_product():
    from streaming_vlm_amd.ops import HipOps
    assert (R.GREEDY, R.GUMBEL, R.FILTERED, R.NUCLEUS) == (HipOps.SAMPLE_GREEDY, HipOps.SAMPLE_GUMBEL, HipOps.SAMPLE_FILTERED, HipOps.SAMPLE_NUCLEUS)
    for k in (0, 1, 2, 50, 2047, 2048, 5000):
        for p in (0.5, 1.0):
            assert R.sample_mode(k, p) == HipOps.sample_mode(k, p)


# ------------------------------------------------------------------------------------------------ the reference run of every case
_RUNS = {}


def ref_run(case):
    if case["name"] not in _RUNS:
        logits, seen0 = SC.materialise(case)
        r = R.replay(case, logits, seen0)
        _RUNS[case["name"]] = {k: r[k] for k in ("tokens", "decided", "min_margin", "max_exp_err", "survivors", "mode", "state", "seen")}
    return _RUNS[case["name"]]


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["name"])
def test_case_meets_the_cap_conditions_with_the_reference_alone(case):
    r = ref_run(case)
    need = R.margin_needed(r["max_exp_err"], case["V"])
    und = int((~r["decided"]).sum())
    print(f"[{case['name']}] margin {r['min_margin']:.3g} (needs {need:.3g}), undecided {und} / {case['n_draws']}, bound_cdf {R.bound_cdf(r['max_exp_err']):.3g}")
    assert r["min_margin"] >= need, "survivor set not decided with 16 x the bound: re-seed or reshape the case"
    assert und <= R.UNDECIDED_CAP * case["n_draws"]
    assert R.bound_cdf(r["max_exp_err"]) <= R.CDF_BOUND_MAX
    assert case["n_draws"] == (300 if case["V"] == SC.FULL_V else 2000)
    assert r["state"] == [case["state"][0] + case["advance_kv"] * case["n_draws"], case["state"][1] + case["n_draws"]]
    if case["check"] == "peak":
        assert set(r["tokens"].tolist()) == {case["V"] // 3}
    if case["check"] == "wide":
        assert int(r["survivors"].sum()) > 2048
    if case["check"] in ("set", "zeros"):
        assert SC.certain_survivors(case) <= set(r["tokens"].tolist())
    if case["name"].startswith("steps8"):
        want = 8 if case["top_p"] == 1.0 else 1 + sum(case["top_p"] > c for c in np.cumsum(SC.STEPS8_MASS)[:-1])
        assert SC.certain_survivors(case) == set(SC.STEPS8_IDS[:want])
    if case["name"].startswith("flatgrid"):
        sc = R.processed(SC.materialise(case)[0], None, 1.0, case["suppress"], R.inv_temp32(case["T"]))
        kth = np.sort(sc)[::-1][case["top_k"] - 1]
        assert int((sc == kth).sum()) >= 3 and int(r["survivors"].sum()) > case["top_k"] and SC.certain_survivors(case) == set(np.nonzero(r["survivors"])[0])
    if case["check"] == "zeros":
        sc = SC.materialise(case)[0]
        kth = np.sort(sc)[::-1][case["top_k"] - 1]
        assert kth == 0 and not np.signbit(kth) and np.signbit(sc[sc == 0]).any()
        assert r["survivors"][(sc == 0) & np.signbit(sc)].all(), "HF keeps -0.0 when the k-th score is +0.0 (-0.0 < +0.0 is false)"


@pytest.mark.parametrize("case", [c for c in SC.CASES if c["V"] < SC.FULL_V], ids=lambda c: c["name"])
def test_survivors_are_the_support_of_the_oracles_warped_softmax(case):
    """survivors64 == support of softmax(oracle.generate.warp_scores(...)) after repetition_penalty and the suppression (first draw)."""
    from oracle import generate as og
    mode = R.sample_mode(case["top_k"], case["top_p"])
    if mode == R.GREEDY:
        return
    logits, seen0 = SC.materialise(case)
    ids = [] if seen0 is None else np.nonzero(seen0)[0].tolist()
    sc = og.repetition_penalty(torch.from_numpy(logits), ids, case["penalty"]).clone()
    if case["suppress"]:
        sc[list(case["suppress"])] = float("-inf")
    # the kernels multiply by fp32 1/T where HF divides by T: the same survivors wherever the margin conditions hold
    w = og.warp_scores(sc * float(R.inv_temp32(case["T"])), 1.0, case["top_k"], case["top_p"])
    want = np.isfinite(w.numpy())                       # what the warpers left unmasked: the support (an exp that underflows is no filter)
    assert (torch.softmax(w.double(), dim=-1).numpy()[~want] == 0).all()
    mine = R.processed(logits, seen0, case["penalty"], case["suppress"], R.inv_temp32(case["T"]))
    mask, margin, _ = R.survivors_of(mode, mine, case["top_k"], case["top_p"])
    assert margin > 0
    assert np.array_equal(mask, want), (int(mask.sum()), int(want.sum()))


# ------------------------------------------------------------------------------------------------ coverage of the case list
def scan_branches(V):
    """The loops of sf_scan a row of V scores runs: whole 4096-vector steps, a clamped last step, the scalar loop (V % 4 != 0)."""
    if V % 4:
        return {"scalar"}
    V4 = V // 4
    return ({"vector"} if V4 >= 4096 else set()) | ({"clamped"} if V4 % 4096 else set())


def descent_depth(case):
    """Levels the filtered kernel's 11 / 11 / 10-bit descent needs: from the keys alone (suppressed ids count with their raw score)."""
    logits, seen0 = SC.materialise(case)
    keys = np.sort(R.sf_key(R.processed(logits, seen0, case["penalty"], None, R.inv_temp32(case["T"]))))[::-1].astype(np.uint64)
    V = case["V"]
    kth = keys[min(min(case["top_k"], V) + len(case["suppress"]), V) - 1]
    for depth, shift in ((1, 21), (2, 10)):
        if int((keys >= ((kth >> np.uint64(shift)) << np.uint64(shift))).sum()) <= 2048:
            return depth
    return 3


def test_case_list_covers_every_mode_scan_branch_and_descent_depth():
    modes, scans, depths = set(), set(), set()
    for c in SC.CASES:
        m = R.sample_mode(c["top_k"], c["top_p"])
        modes.add(m)
        if m in (R.FILTERED, R.NUCLEUS):
            scans |= {(m, b) for b in scan_branches(c["V"])}
        if m == R.FILTERED:
            depths.add(descent_depth(c))
    assert modes == {R.GREEDY, R.GUMBEL, R.FILTERED, R.NUCLEUS}
    assert scans == {(m, b) for m in (R.FILTERED, R.NUCLEUS) for b in ("scalar", "clamped", "vector")}, scans
    assert depths == {1, 2, 3}, depths
    assert scan_branches(4096) == {"clamped"} and scan_branches(16384) == {"vector"} and scan_branches(16388) == {"vector", "clamped"}
    by_mode = {m: {c["V"] for c in SC.CASES if R.sample_mode(c["top_k"], c["top_p"]) == m} for m in modes}
    assert all(SC.FULL_V in by_mode[m] for m in modes)
    assert {1, 2, 3, 130, 3001, 4096, 16384, 16388, 20000} <= by_mode[R.FILTERED] | by_mode[R.NUCLEUS]
    ks = {(c["top_k"], c["top_p"]) for c in SC.CASES}
    assert {(2, 1.0), (50, 1.0), (2047, 1.0), (0, 0.5), (0, 0.95), (2048, 1.0), (2048, 0.9), (5000, 1.0), (5000, 0.9)} <= ks
    assert {c["T"] for c in SC.CASES} >= {1e-3, 0.7, 4.0} and {c["state"] for c in SC.CASES} >= {(0, -1), (977, 1000)}
    assert {len(c["suppress"]) for c in SC.CASES} >= {0, 2, 8} and {c["advance_kv"] for c in SC.CASES} == {0, 1}
    for c in SC.CASES:
        if c["suppress"]:
            logits, seen0 = SC.materialise(c)
            assert int(np.argmax(logits)) == c["suppress"][0]
            assert seen0 is None or len(c["suppress"]) < 3 or seen0[c["suppress"][2]]


# ------------------------------------------------------------------------------------------------ fp32 emulation of the kernels' arithmetic
def exp32(d):
    """__expf in fp32: exp2(fl(log2e) * d), every step rounded to fp32."""
    return np.exp2((F32(1.4426950408889634) * d.astype(F32)).astype(F32)).astype(F32)


def gumbel32(seed, step, idx, swap=False):
    vv = R.gumbel_vv(seed, step, idx, swap)
    with np.errstate(divide="ignore"):
        return (-np.log((-np.log1p(-vv)).astype(F32))).astype(F32)


def am_best(val, idx):
    val = np.where(np.isnan(val), -np.inf, val)
    ok = val > -np.inf
    if not ok.any():
        return 0
    return int(idx[np.lexsort((idx, -val))[0]])


def emulate_draw(mode, case, logits, seen, step, fault=None):
    """One draw in the kernels' fp32 arithmetic (not their radix machinery).  `fault`: one of FAULTS."""
    V = case["V"]
    inv_t = F32(1.0) if mode == R.GREEDY else R.inv_temp32(case["T"])
    sup = np.array(case["suppress"] or (), dtype=np.int64)
    if fault == "penalty_after_temp":
        sc = R.processed(R.processed(logits, None, 1.0, None, inv_t), seen, case["penalty"], sup, F32(1.0))
    else:
        sc = R.processed(logits, seen, case["penalty"], sup, inv_t)
    idx = np.arange(V)
    if mode == R.GREEDY:
        return am_best(sc, idx)
    swap = fault == "counter_swapped"
    if mode == R.GUMBEL:
        g = gumbel32(case["seed"], step, idx, swap)
        return am_best((sc + (g * inv_t if fault == "temp_on_noise" else g)).astype(F32), idx)
    keys = R.sf_key(sc).astype(np.int64)
    top_k, top_p = case["top_k"], F32(case["top_p"])
    if mode == R.FILTERED:
        alive = idx[sc > -np.inf]
        tie = alive if fault != "high_index_first" else -alive
        cand = alive[np.lexsort((tie, -keys[alive]))]
        n = min(min(top_k, V), cand.size)
        if fault == "suppress_in_k" and sup.size:
            raw = R.processed(logits, seen, case["penalty"], None, inv_t)
            n = max(1, n - int(np.isin(np.argsort(-raw, kind="stable")[:n], sup).sum())) if cand.size else 0
        if n == 0:
            return 0
        if fault != "ties_dropped":
            while n < cand.size and keys[cand[n]] == keys[cand[n - 1]]:
                n += 1
        P = 64
        while P < n:
            P <<= 1
        s = sc[cand[:n]] + F32(0.0)
        f = np.zeros(P, dtype=F32)
        f[:n] = exp32(s - s[0])
        off = 1
        while off < P:                                   # the inclusive prefix-sum tree
            f[off:] = f[off:] + f[:-off].copy()
            off <<= 1
        total, keep = f[n - 1], n
        if top_p < F32(1.0):
            lo, hi = 1, n
            while lo < hi:
                mid = (lo + hi) >> 1
                if F32(total - f[mid - 1]) <= F32(F32(F32(1.0) - top_p) * total):
                    hi = mid
                else:
                    lo = mid + 1
            keep = lo
            if fault == "keep_plus_1":
                keep = min(n, keep + 1)
            if fault == "keep_minus_1":
                keep = max(1, keep - 1)
        u = F32(R.uniform(case["seed"], step) * f[keep - 1])
        lo, hi = 0, keep - 1
        while lo < hi:
            mid = (lo + hi) >> 1
            if f[mid] > u:
                hi = mid
            else:
                lo = mid + 1
        return int(cand[lo])
    # ---- nucleus: thresholds on the key, by count and by 2^-40 fixed-point mass
    smax = sc.max()
    tau = 0
    if 0 < top_k < V:
        k = top_k
        tau = int(np.sort(keys)[::-1][k - 1])
        if fault == "suppress_in_k" and sup.size:
            tau = int(np.sort(R.sf_key(R.processed(logits, seen, case["penalty"], None, inv_t)).astype(np.int64))[::-1][k - 1])
        if fault == "ties_dropped":
            tau += 1 if int((keys >= tau).sum()) > top_k else 0
    if top_p < F32(1.0):
        sel = keys >= tau
        with np.errstate(over="ignore"):
            m = np.where(sel, (exp32(sc - smax) * F32(1099511627776.0)).astype(np.float64), 0.0).astype(np.uint64)
        target = int(np.float64(top_p) * np.float64(int(m.sum())))
        uk, inv = np.unique(keys, return_inverse=True)
        mk = np.bincount(inv, weights=m.astype(np.float64), minlength=uk.size)[::-1]      # exact: sums stay below 2^53
        acc = np.cumsum(mk)
        j = int(np.argmax(acc >= target))
        if fault == "keep_plus_1":
            j = min(j + 1, uk.size - 1)
        if fault == "keep_minus_1":
            j = max(j - 1, 0)
        tau = max(tau, int(uk[::-1][j]))
    live = idx[(keys >= tau) & (sc > -np.inf)]
    g = gumbel32(case["seed"], step, live, swap)
    return am_best((sc[live] + (g * inv_t if fault == "temp_on_noise" else g)).astype(F32), live)


FAULTS = ["keep_plus_1", "keep_minus_1", "ties_dropped", "suppress_in_k", "penalty_after_temp", "step_not_plus_1", "counter_swapped",
          "high_index_first", "seen_not_updated", "temp_on_noise"]


def emulate_and_compare(case, fault=None, n_draws=None):
    """The emulation run as the product runs the kernels, replayed by the reference -> (mismatches on decided draws, drawn-set or
    final-state violations)."""
    logits, seen0 = SC.materialise(case)
    c = dict(case, n_draws=n_draws or case["n_draws"])
    mode = R.sample_mode(c["top_k"], c["top_p"])
    seen = None if seen0 is None else seen0.copy()
    cur, toks = c["state"][1], []
    for _ in range(c["n_draws"]):
        t = emulate_draw(mode, c, logits, seen, cur + (0 if fault == "step_not_plus_1" else 1), fault)
        toks.append(t)
        if seen is not None and fault != "seen_not_updated":
            seen[t] = 1
        cur += 1
    toks = np.array(toks)
    ref = R.replay(c, logits, seen0, gpu_tokens=toks)
    bad = int((ref["decided"] & (ref["tokens"] != toks)).sum())
    other = int(seen is not None and not np.array_equal(seen, ref["seen"]))
    if ref["survivors"] is not None:
        other += int(not set(toks.tolist()) <= set(np.nonzero(ref["survivors"])[0].tolist()))
    if c["check"] in ("set", "zeros") and n_draws is None:
        other += int(not SC.certain_survivors(case) <= set(toks.tolist()))
    return bad, other


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: c["name"])
def test_emulation_agrees_on_every_decided_draw(case):
    big = case["V"] > 3001 and R.sample_mode(case["top_k"], case["top_p"]) in (R.GUMBEL, R.NUCLEUS)
    bad, other = emulate_and_compare(case, n_draws=100 if big else None)       # Philox over a wide nucleus twice: the first 100 draws
    assert (bad, other) == (0, 0)


@pytest.mark.parametrize("fault", FAULTS)
def test_injected_fault_is_caught(fault):
    """Each fault, put into the emulation, makes at least one case fail (a decided draw differs, or a drawn-set / seen check does)."""
    caught = []
    for case in SMALL:
        bad, other = emulate_and_compare(case, fault, n_draws=None if case["check"] else 300)
        if bad or other:
            caught.append((case["name"], bad, other))
            break
    print(f"[fault {fault}] caught by {caught}")
    assert caught, f"no case notices `{fault}`"
