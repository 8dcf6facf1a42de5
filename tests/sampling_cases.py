"""The case list of the exact sampling replay (tests/test_sampling_ref64.py on the host, tests/test_sampling_replay_gpu.py on the GPU).

A case: V, a logits generator (+ its seed), `seen` density (None: no seen buffer is passed, so nothing is marked either), penalty,
suppress list, T, top_k, top_p, rng seed, start `state`, advance_kv, n_draws.  materialise(case) -> (logits fp32, seen0 uint8 | None).
Small vocabularies draw 2000 tokens, the full vocabulary 300.  Conditions every case must meet WITH THE REFERENCE ALONE (asserted in
the host tests): survivor margin >= 16 x the bound, at most 1 % undecided draws."""
import functools
import math

import numpy as np
import torch

FULL_V = 151936
STEPS8_MASS = (0.40, 0.20, 0.15, 0.10, 0.06, 0.04, 0.03, 0.02)
STEPS8_IDS = (5, 0, 63, 64, 17, 129, 100, 2)               # where the eight heavy tokens sit (V >= 130)
STEPS8_TOP_P = (0.20, 0.50, 0.675, 0.80, 0.88, 0.93, 0.965)   # midpoints of 0, .40, .60, .75, .85, .91, .95, .98: 1..7 survivors


def _zeros_logits(V, n_above, n_pos0, n_neg0):
    """n_above scores above zero, then +0.0 / -0.0 entries (-0.0 first by index), the rest negative."""
    x = -1.0 - np.arange(V, dtype=np.float32) * np.float32(0.001)
    x[1:1 + n_neg0] = -0.0
    x[1 + n_neg0:1 + n_neg0 + n_pos0] = 0.0
    x[V - n_above:] = 0.5 + np.arange(n_above, dtype=np.float32) * np.float32(0.001)
    return x


def _penalty_tie(penalty, T):
    """Two neighbouring fp32 values a < b with fl(fl(a / p) * t) == fl(fl(b / p) * t) but fl(fl(a * t) / p) != fl(fl(b * t) / p):
    seen both, they tie only when the penalty comes before the temperature (mathematically the two orders are the same number)."""
    p, t = np.float32(penalty), np.float32(1.0) / np.float32(T)
    a = (np.float32(1.5).view(np.uint32) + np.arange(1 << 16, dtype=np.uint32)).view(np.float32)
    b = (a.view(np.uint32) + np.uint32(1)).view(np.float32)
    hit = np.nonzero(((a / p) * t == (b / p) * t) & ((a * t) / p != (b * t) / p))[0]
    return a[hit[0]], b[hit[0]]


def _logits(gen, V, seed, T):
    if gen == "ptie":                                     # V = 16, everything seen: token 3 tops, 9 and 5 tie for the second place
        x = -2.0 - np.arange(V, dtype=np.float32) * np.float32(0.25)
        x[9], x[5] = _penalty_tie(1.3, T)
        x[3] = 2.5
        return x
    if gen == "zeros16":                                  # k = 3: two scores above, the third is a zero; 5 zeros tie
        return _zeros_logits(16, 2, 2, 3)
    if gen == "zeros2600":                                # k = 2100: the 2100th largest is a zero; 50 zeros tie
        return _zeros_logits(2600, 2090, 20, 30)
    g = torch.Generator().manual_seed(seed)
    if gen == "iid":
        x = torch.randn(V, generator=g) * 2.0
    elif gen == "head":                                   # 40 live tokens, the rest 30 below: a full-width scan whose nucleus boundary
        x = torch.randn(V, generator=g) * 2.0 - 30.0      # stays 16 bounds away from top_p through 300 draws of live feedback
        h = torch.randperm(V, generator=g)[:40]
        x[h] += 30.0
    elif gen == "grid":                                   # multiples of 0.25: exact ties at the k-th score and elsewhere
        x = torch.round(torch.randn(V, generator=g) * 4.0) / 4.0
    elif gen == "flatgrid":                               # few levels, flat: every tie of a small V holds >= 1 % of the mass
        x = torch.randint(0, 4, (V,), generator=g).float() * 0.25
    elif gen == "onebin":                                 # [8, 8.99): one 11-bit radix bin
        x = 8.0 + torch.rand(V, generator=g) * 0.99
    elif gen == "dense":                                  # ~1000 neighbouring fp32 values: one bin on two levels, third level decides
        x = 8.0 + torch.rand(V, generator=g) * 9e-4
    elif gen == "signed":                                 # symmetric, many negatives, exact +0.0 and -0.0 entries
        x = torch.randn(V, generator=g) * 3.0
        z = torch.randperm(V, generator=g)[:max(2, V // 8)]
        x[z[0::2]] = 0.0
        x[z[1::2]] = -0.0
    elif gen == "peaked":                                 # one token holds > 0.99 of the mass (after the temperature)
        x = torch.randn(V, generator=g) * 0.5 * T
        x[V // 3] = (math.log(V) + 8.0) * T
    elif gen == "flat":                                   # nucleus of thousands: 3000 near-equal tokens, the rest 25 below (a wider
        x = torch.randn(V, generator=g) * 0.05            # one cannot keep its boundary token 16 bounds away from the threshold)
        x[torch.randperm(V, generator=g)[3000:]] -= 25.0
    elif gen == "far":                                    # everything but the peak 120 below: exp underflows, the fixed-point mass is 0
        x = torch.randn(V, generator=g) * 0.5 * T - 120.0 * T
        x[V // 3] = 0.0
    elif gen == "steps8":                                 # eight tokens with STEPS8_MASS after the temperature, the rest 40 below
        x = torch.full((V,), (math.log(STEPS8_MASS[0]) - 40.0) * T) + torch.rand(V, generator=g) * 0.01 * T
        for i, m in zip(STEPS8_IDS, STEPS8_MASS):
            x[i] = math.log(m) * T
    else:
        raise ValueError(gen)
    return x.float().numpy().copy()


@functools.lru_cache(maxsize=4)
def _materialise(name):
    c = BY_NAME[name]
    logits = _logits(c["gen"], c["V"], c["gen_seed"], c["T"])
    seen = None
    if c["seen"] is not None:
        g = torch.Generator().manual_seed(c["gen_seed"] + 1)
        seen = (torch.rand(c["V"], generator=g) < c["seen"]).to(torch.uint8).numpy().copy()
        for s in c["suppress"][2:3]:                      # the third suppressed id (when there is one) is also seen
            seen[s] = 1
    return logits, seen


def materialise(case):
    logits, seen = _materialise(case["name"])
    return logits.copy(), None if seen is None else seen.copy()


def _suppress(gen, V, gen_seed, T, n):
    """n ids: the raw argmax, ids inside the top of the row, and (third) one that materialise() also marks seen."""
    if n == 0:
        return ()
    order = np.argsort(-_logits(gen, V, gen_seed, T), kind="stable")
    picks = [0, 2, 5, 1, 7, 3, 11, 4][:n]
    return tuple(int(order[min(p, V - 1)]) for p in picks)


def certain_survivors(case):
    """The survivors that `n_draws` draws cannot miss (P(never drawn) < 1e-12), from the reference alone; cases without feedback."""
    import sampling_ref64 as R
    assert case["seen"] is None
    logits, _ = materialise(case)
    mode = R.sample_mode(case["top_k"], case["top_p"])
    sc = R.processed(logits, None, 1.0, case["suppress"], R.inv_temp32(case["T"]))
    _, _, info = R.survivors_of(mode, sc, case["top_k"], case["top_p"])
    p = info["w"] / info["w"].sum()
    return set(int(t) for t in info["order"][case["n_draws"] * np.log1p(-np.minimum(p, 0.5)) < np.log(1e-12)])


CASES = []


def _case(name, V, gen, top_k, top_p, T=0.7, seen=None, penalty=1.0, n_sup=0, seed=(12345, 678), state=(0, -1), advance_kv=0,
          n_draws=None, gen_seed=None, check=None):
    gen_seed = gen_seed if gen_seed is not None else (V * 7 + len(CASES))
    CASES.append(dict(name=name, V=V, gen=gen, gen_seed=gen_seed, seen=seen, penalty=penalty,
                      suppress=_suppress(gen, V, gen_seed, T, n_sup), T=T, top_k=top_k, top_p=top_p, seed=seed, state=tuple(state),
                      advance_kv=advance_kv, n_draws=n_draws or (300 if V >= 100000 else 2000), check=check))


def _build():
    # ---- 1. vocabulary sizes x kernels (sf_scan: scalar only / one clamped vector step / one full step / full + clamped)
    for V in (1, 2, 3):
        _case(f"V{V}-gumbel", V, "iid", 0, 1.0)
        _case(f"V{V}-filtered-k2", V, "iid", 2, 1.0)                       # k >= V
        _case(f"V{V}-nucleus-p0.5", V, "iid", 0, 0.5)
    for V in (130, 3001):
        _case(f"V{V}-greedy", V, "iid", 1, 1.0, seen=0.3, penalty=1.3)
        _case(f"V{V}-gumbel", V, "iid", 0, 1.0, T=4.0, seen=0.3, penalty=1.05, n_sup=2, state=(977, 1000), advance_kv=1)
        _case(f"V{V}-filtered-k50-p0.9", V, "iid", 50, 0.9, seen=0.1, penalty=1.05, n_sup=2, gen_seed=1)      # seeds: searched for the margin
        _case(f"V{V}-nucleus-p0.95", V, "iid", 0, 0.95, state=(977, 1000), advance_kv=1, gen_seed=2)
    for V in (4096, 16384, 16388):
        _case(f"V{V}-filtered-k50", V, "iid", 50, 1.0, n_sup=2)
        _case(f"V{V}-nucleus-p0.5", V, "iid", 0, 0.5)
    _case("V20000-filtered-k2", 20000, "iid", 2, 1.0)
    _case("V20000-filtered-k2047", 20000, "iid", 2047, 1.0, T=4.0)
    _case("V20000-nucleus-k2048-p1", 20000, "iid", 2048, 1.0, T=4.0)
    _case("V20000-nucleus-k2048-p0.9", 20000, "iid", 2048, 0.9, T=4.0)
    _case("V20000-nucleus-k5000-p1", 20000, "iid", 5000, 1.0, T=4.0, n_sup=8)
    _case("V20000-nucleus-k5000-p0.9", 20000, "iid", 5000, 0.9, T=4.0)
    _case("V3001-nucleus-k3001", 3001, "iid", 3001, 0.9)                    # k >= V in the nucleus kernel: no count threshold
    _case("V3001-nucleus-k2048-grid", 3001, "grid", 2048, 1.0, T=4.0)       # ties at the k-th of the count descent
    _case("V12-filtered-k6-sup8", 12, "iid", 6, 1.0, n_sup=8, check="set")  # k larger than the number of finite scores (4)
    _case("V12-nucleus-sup8", 12, "iid", 0, 0.95, n_sup=8)
    for mode, k, p, gen in (("greedy", 1, 1.0, "iid"), ("gumbel", 0, 1.0, "iid"), ("filtered-k50-p0.9", 50, 0.9, "iid"), ("nucleus-p0.95", 0, 0.95, "head")):
        _case(f"full-{mode}", FULL_V, gen, k, p, T=0.9, gen_seed=1, seen=0.003, penalty=1.05, n_sup=2, state=(977, 1000), advance_kv=1)
    # ---- 3. steps8: the survivor count runs 1..8 in both kernels; the drawn set must be the survivor set
    for kern, k in (("filtered", 50), ("nucleus", 0)):
        for p in STEPS8_TOP_P + (0.99,):
            _case(f"steps8-{kern}-p{p}", 130, "steps8", k, p, check="set")
    _case("steps8-filtered-p1", 130, "steps8", 50, 1.0, check="set")
    # ---- 4. ties of the k-th score survive
    _case("flatgrid-k5-ties", 24, "flatgrid", 5, 1.0, T=1.0, check="set")
    _case("flatgrid-k5-ties-sup", 24, "flatgrid", 5, 1.0, T=1.0, n_sup=2, check="set")
    # ---- 5. suppress does not consume places of k
    _case("sup2-filtered-k4", 130, "iid", 4, 1.0, T=4.0, n_sup=2, check="set")
    _case("sup8-filtered-k4", 130, "iid", 4, 1.0, T=4.0, seen=0.1, penalty=1.05, n_sup=8)
    _case("sup8-nucleus-p0.5", 130, "iid", 0, 0.5, T=4.0, n_sup=8)
    # ---- 6. penalty before temperature, flipping on the sign; live seen feedback
    for kern, k, p in (("gumbel", 0, 1.0), ("filtered", 20, 1.0), ("nucleus", 0, 0.9)):
        _case(f"penalty-{kern}", 130, "signed", k, p, T=0.5, seen=0.3, penalty=1.3)
    _case("penalty-order-tie", 16, "ptie", 2, 1.0, T=0.7, seen=1.0, penalty=1.3)
    # ---- 7. temperatures, start states, advance_kv
    _case("T1e-3-filtered", 3001, "iid", 50, 0.9, T=1e-3, state=(977, 1000), advance_kv=1)
    _case("T1e-3-gumbel", 130, "iid", 0, 1.0, T=1e-3)
    _case("T4-filtered", 3001, "iid", 50, 1.0, T=4.0, state=(977, 1000), advance_kv=1)
    # ---- 8. multi-level descent
    _case("onebin-k50", 20000, "onebin", 50, 1.0, T=0.9)
    _case("dense-k50", 20000, "dense", 50, 1.0, T=1.0)
    # ---- 9. a nucleus of more than 2048 survivors
    _case("flat-nucleus-p0.9", 20000, "flat", 0, 0.9, T=1.0, check="wide")
    # ---- 10. far and peaked: every draw is the peak
    for gen in ("far", "peaked"):
        _case(f"{gen}-filtered", 3001, gen, 50, 0.9, check="peak")
        _case(f"{gen}-nucleus", 3001, gen, 0, 0.9, check="peak")
    # ---- signed zeros: the k-th score is +0.0 with -0.0 entries present (HF: -0.0 >= +0.0 survives)
    _case("zeros-filtered-k", 16, "zeros16", 3, 1.0, T=1.0, check="zeros")
    _case("zeros-nucleus-k", 2600, "zeros2600", 2100, 1.0, T=1.0, check="zeros")


_build()
BY_NAME = {c["name"]: c for c in CASES}
assert len(BY_NAME) == len(CASES)
