"""Exact host replay of the device-side token choice (test helper; numpy only, no GPU).

Everything after the fp32 logits row is a deterministic function of (rng seed, state[1], logits, seen, suppress): the noise is
Philox4x32-10 counted by (vocabulary index | 0xFFFFFFFF, index of the token being chosen).  This module restates that function
independently of the kernels' machinery (no radix descent, no candidate list, no bitonic sort, no fixed point): HF's survivor rule and
the draw in float64 on the kernels' exact fp32 processed scores, and says for every draw whether the float64 answer is DECIDED, i.e.
farther from the nearest decision boundary than the fp32 arithmetic of the kernels can move it.  A decided draw must equal the
kernel's token; an undecided one is skipped (and counted: the case list caps them at 1 % per case).

What is exact and what is bounded
---------------------------------
* Philox, the uniform `((x >> 9) + 0.5) * 2^-23` and `vv = (float32(x) + 0.5f) * 2^-32` are integer / single fp32 operations: numpy
  reproduces their bits.  So are the processed scores: penalty (`x < 0 ? x * p : x / p`), -inf at suppressed ids, `* inv_temp` with
  `inv_temp = float32(1) / float32(T)`.  Top-k compares those fp32 scores: exact, no margin.
* Accuracy of the device math functions.  No accuracy table ships with the toolchain (the device-library package installs its licence
  only), so the figures are ASSUMED from the published limits the library is built to: OpenCL full profile for `log` (3 ulp) and
  `log1p` (2 ulp), and 1 ulp for the hardware `exp2` behind `__expf(x) = exp2(fl(log2e) * x)`.  1 ulp <= 2^-23 relative.  Every
  assumed figure is multiplied by SLACK = 4 (a documented limit, not a measurement; slack only costs undecided draws).  None of
  them is taken from the kernels' output.

bound_cdf (filtered kernel: inverse CDF over the sorted survivors), relative to the survivors' total weight W = C[keep-1]:
    e_i = __expf(s_i - s_0), D_i = s_0 - s_i >= 0:
      fp32 rounding of the difference            2^-24 D_i            (absolute, in the exponent = relative in e_i)
      fl(log2e) and fl(log2e * d)                2 * 2^-24 D_i
      exp2 itself                                2^-23
      -> rel(e_i) <= SLACK * 2^-24 * (2 + 3 D_i)       [derived from the algorithm: the error grows with |s_i - s_0|]
    prefix-sum tree: log2(P) <= 11 fp32 additions on partial sums <= W           11 * 2^-24
    r = u * W (u is exact)                                                        1 * 2^-24
    bound_cdf = [ sum_i e_i * SLACK * (2 + 3 D_i) / W + 12 ] * 2^-24
  The first term is a weighted mean over the survivors (e_i D_i <= 1/e, so far-away tokens add nothing); it is evaluated per draw.
  Over the case list it stays below CDF_BOUND_MAX = 64 * 2^-24 = 3.8e-6 (asserted on the host).
  The same bound (+ 3 * 2^-24 for `total - prefix`, `1 - top_p` and their product) moves the kernel's top-p cut.

bound_gumbel (Gumbel-max kernels: argmax of s_i + g_i), absolute, per candidate:
    g = -logf(E), E = -log1pf(-vv):  E carries 2 ulp of log1p -> shifts g by 2 * 2^-23;  logf adds 3 ulp of |g|
      -> |dg| <= SLACK * 2^-23 * (2 + 3 |g|)
    the score: the reference adds the ROUNDED fp32 product x * inv_temp; the compiler may contract `x * inv_temp + g` into one fma,
      which adds the unrounded product                                         2^-24 |s|
    one fp32 rounding of the sum                                               2^-24 |s + g|
    bound_gumbel_i = SLACK * 2^-23 * (2 + 3 |g_i|) + 2^-24 (|s_i| + |s_i + g_i|)
  (|g| <= 25: about 3.7e-5 at the very tail, 5e-6 for a typical winner.)  A draw is decided iff the winner, lowered by its bound,
  still beats every other survivor raised by its own.

Nucleus threshold (nucleus kernel: masses in 2^-40 fixed point): each mass is truncated by < 2^-40 of the largest one, V of them, so
the margin of the survivor set has to exceed the weighted exp error above PLUS V * 2^-40.

Survivor margin: the smallest relative distance |X_j / Z - top_p| / top_p over the sorted entries j >= 1 (X_j = weight of the entries
in front of j).  The case list requires margin >= 16 x (bound_cdf + 3 * 2^-24 + V * 2^-40), so neither kernel's cut can move.  A group
of equal scores that the threshold falls inside (HF cuts it by sort position, the nucleus kernel keeps it whole) has margin 0.
"""
import numpy as np

GREEDY, GUMBEL, FILTERED, NUCLEUS = 0, 1, 2, 3          # HipOps.SAMPLE_*
MODE_NAMES = {GREEDY: "greedy", GUMBEL: "gumbel", FILTERED: "filtered", NUCLEUS: "nucleus"}

SLACK = 4.0
U24 = 2.0 ** -24
CDF_BOUND_MAX = 64 * U24
MARGIN_FACTOR = 16.0
UNDECIDED_CAP = 0.01

# literals of csrc/common.h (pinned on the source in tests/test_sampling_ref64.py)
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
UNIFORM_IDX = 0xFFFFFFFF
UNIFORM_SHIFT, UNIFORM_SCALE = 9, 1.0 / 8388608.0
GUMBEL_SCALE = 1.0 / 4294967296.0
M32 = np.uint64(0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ Philox4x32-10
def philox4(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11), all four output words; vectorised over any of the counter words (exact: uint64)."""
    c = [np.asarray(x, dtype=np.uint64) & M32 for x in (c0, c1, c2, c3)]
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]
        c = [(p1 >> s32) ^ c[1] ^ np.uint64(k0), p1 & M32, (p0 >> s32) ^ c[3] ^ np.uint64(k1), p0 & M32]
        k0, k1 = (k0 + PHILOX_W0) & 0xFFFFFFFF, (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c


def philox_first(c0, c1, k0, k1):
    """svlm_philox_first: counter (c0, c1, 0, 0), word 0."""
    return philox4(c0, c1, 0, 0, k0, k1)[0]


def uniform(seed, step):
    """svlm_philox_uniform(rng, step, 0xFFFFFFFF): 23 random bits + 1/2, exact in fp32."""
    x = int(philox_first(UNIFORM_IDX, int(step) & 0xFFFFFFFF, seed[0], seed[1]))
    return np.float32((np.float32(x >> UNIFORM_SHIFT) + np.float32(0.5)) * np.float32(UNIFORM_SCALE))


def gumbel_vv(seed, step, v, swap=False):
    """The fp32 uniform the Gumbel noise is made from, bit for bit: (float32(x) + 0.5f) * 2^-32.  `swap`: counter words exchanged
    (an injected fault of the emulation)."""
    v = np.asarray(v, dtype=np.uint64)
    st = np.uint64(int(step) & 0xFFFFFFFF)
    x = philox_first(st, v, *seed) if swap else philox_first(v, st, *seed)
    return (x.astype(np.float32) + np.float32(0.5)) * np.float32(GUMBEL_SCALE)


def gumbel64(seed, step, v):
    """Standard Gumbel noise of vocabulary entries `v` at `step`: -log(-log1p(-vv)) in float64 on the kernel's fp32 vv (-inf at vv = 1)."""
    vv = gumbel_vv(seed, step, v).astype(np.float64)
    with np.errstate(divide="ignore"):
        return -np.log(-np.log1p(-vv))


# ------------------------------------------------------------------------------------------------ processed scores, keys
def inv_temp32(temperature):
    return np.float32(1.0) / np.float32(temperature)


def processed(logits_f32, seen, penalty, suppress, inv_temp_f32):
    """The kernels' fp32 processed scores: repetition penalty where seen, -inf at suppressed ids, then * inv_temp."""
    x = np.asarray(logits_f32, dtype=np.float32).copy()
    if seen is not None:
        m = np.asarray(seen) != 0
        p = np.float32(penalty)
        x[m] = np.where(x[m] < 0, x[m] * p, x[m] / p)
    if suppress is not None and len(suppress):
        x[np.asarray(suppress, dtype=np.int64)] = -np.inf
    return x * np.float32(inv_temp_f32)


def sf_key(scores_f32):
    """Order-preserving float -> uint32 of csrc/dec_sample.h (the zero is canonicalised first: -0.0 and +0.0 share a key)."""
    u = (np.asarray(scores_f32, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u >> np.uint32(31), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


# ------------------------------------------------------------------------------------------------ survivors (HF's rule, float64)
def survivors64(scores, top_k, top_p, sort=True):
    """-> (mask, margin, info).  top-k keeps every score >= the k-th largest (k = min(k, V); ties survive); then a token survives
    top-p iff the softmax mass of the strictly larger scores (among the top-k survivors) is < top_p; the largest always survives.
    margin: smallest relative distance of a sorted entry's leading mass from top_p (inf when top_p = 1), 0 when the threshold falls
    inside a group of equal scores.  info: order (survivors, score descending, lowest index first), weights exp(s - s0), exp_err (the
    weighted exp term of bound_cdf, in units of 2^-24) over the top-k survivors."""
    s = np.asarray(scores, dtype=np.float64)
    V = s.size
    mask = s > -np.inf
    if top_k and top_k > 0:
        k = min(int(top_k), V)
        kth = np.partition(s, V - k)[V - k]
        mask &= s >= kth
    elif top_p < 1.0 and V > 1:                          # nothing 60 below the maximum can survive top-p alone (e^-60 V << 2^-53): not sorted
        mask &= s >= s.max() - 60.0
    idx = np.nonzero(mask)[0]
    if not sort:                                         # Gumbel-max over everything finite: no order needed (top_k = 0, top_p = 1)
        assert not top_k and top_p >= 1.0
        D = (s[idx].max() - s[idx]) if idx.size else np.zeros(0)
        return mask, np.inf, dict(order=idx, w=np.exp(-D), exp_err=0.0)
    order = idx[np.lexsort((idx, -s[idx]))]
    if order.size == 0:                                  # every score -inf: the kernels answer token 0
        return mask, np.inf, dict(order=order, w=np.zeros(0), exp_err=0.0)
    so = s[order]
    D = so[0] - so
    w = np.exp(-D)
    margin = np.inf
    if top_p < 1.0:
        Z = w.sum()
        X = np.concatenate(([0.0], np.cumsum(w)[:-1])) / Z            # mass in front of each sorted entry
        first = np.concatenate(([True], so[1:] != so[:-1]))           # first entry of each group of equal scores
        grp = np.maximum.accumulate(np.where(first, np.arange(so.size), 0))
        top_p = np.float64(np.float32(top_p))                        # the kernels hold top_p in fp32
        keep = X[grp] < top_p                                         # by the strictly larger scores
        keep[0] = True
        if so.size > 1:
            margin = float(np.min(np.abs(X[1:] - top_p)) / top_p)
            if np.any(keep[1:] != (X[1:] < top_p)):                   # the threshold falls inside a tie
                margin = 0.0
        mask = np.zeros(V, dtype=bool)
        mask[order[keep]] = True
        order, w, D = order[keep], w[keep], D[keep]
    exp_err = float(np.sum(w * SLACK * (2.0 + 3.0 * D)) / np.sum(w))
    return mask, margin, dict(order=order, w=w, exp_err=exp_err)


def bound_cdf(exp_err):
    return (exp_err + 12.0) * U24


def margin_needed(exp_err, V):
    return MARGIN_FACTOR * (bound_cdf(exp_err) + 3 * U24 + V * 2.0 ** -40)


def bound_gumbel(s, g):
    return SLACK * 2 * U24 * (2.0 + 3.0 * np.abs(g)) + U24 * (np.abs(s) + np.abs(s + g))


# ------------------------------------------------------------------------------------------------ one draw
def sample_mode(top_k, top_p):
    """HipOps.sample_mode restated (pinned against it in the host tests)."""
    if int(top_k) == 1:
        return GREEDY
    if int(top_k) == 0 and float(top_p) >= 1.0:
        return GUMBEL
    return NUCLEUS if (int(top_k) == 0 or int(top_k) >= 2048) else FILTERED


def survivors_of(mode, scores, top_k, top_p):
    return survivors64(scores, 0, 1.0, sort=False) if mode == GUMBEL else survivors64(scores, top_k, top_p)


def expected(mode, scores, top_k, top_p, seed, step, surv=None):
    """-> dict(token, decided, dist, margin, order, prob): the float64 draw at `step` from fp32 processed `scores`.
    dist: distance to the nearest decision boundary in units of the bound (> 1 = decided).  prob(token) -> reference probability."""
    if mode == GREEDY:
        tok = int(np.argmax(scores)) if np.any(scores > -np.inf) else 0
        return dict(token=tok, decided=True, dist=np.inf, margin=np.inf, order=np.array([tok]), prob=lambda t: float(t == tok))
    if surv is None:
        surv = survivors_of(mode, scores, top_k, top_p)
    mask, margin, info = surv
    order, w = info["order"], info["w"]
    Z = w.sum() if order.size else 1.0

    def prob(t):
        j = np.nonzero(order == t)[0]
        return float(w[j[0]] / Z) if j.size else 0.0

    out = dict(margin=margin, order=order, prob=prob, exp_err=info["exp_err"])
    if order.size == 0:
        return dict(out, token=0, decided=True, dist=np.inf)
    if mode == FILTERED:
        C = np.cumsum(w)
        r = np.float64(uniform(seed, step)) * C[-1]
        i = int(np.searchsorted(C[:-1], r, side="right"))            # first i with C_i > r; the last entry takes the rest
        b = bound_cdf(info["exp_err"]) * C[-1]
        d = float(np.min(np.abs(C[:-1] - r))) / b if C.size > 1 else np.inf
        return dict(out, token=int(order[i]), decided=d > 1.0, dist=d)
    s = np.asarray(scores, dtype=np.float64)[order]
    g = gumbel64(seed, step, order)
    val = s + g
    val = np.where(np.isnan(val), -np.inf, val)
    top = int(np.lexsort((order, -val))[0])                           # largest value, lowest index among equals
    if order.size == 1:
        return dict(out, token=int(order[top]), decided=True, dist=np.inf)
    e = bound_gumbel(s, np.where(np.isfinite(g), g, 0.0))
    rest = np.delete(np.arange(order.size), top)
    gap = (val[top] - val[rest])
    with np.errstate(invalid="ignore"):
        d = float(np.min(np.where(np.isfinite(val[rest]), gap / (e[top] + e[rest]), np.inf))) if np.isfinite(val[top]) else 0.0
    return dict(out, token=int(order[top]), decided=d > 1.0, dist=d)


# ------------------------------------------------------------------------------------------------ a sequence of draws
def replay(case, logits, seen0, gpu_tokens=None, detail_at=None):
    """`n_draws` consecutive draws as the product does them: step = state[1] + 1, the drawn token marked in `seen` (when the case
    has a seen buffer), state[1] += 1, state[0] += advance_kv.  With `gpu_tokens` the sequence follows the kernel's tokens (so an
    undecided draw does not invalidate what comes after it).
    -> dict(tokens, decided (bool array), dist, seen, state, min_margin, max_exp_err, survivors (union over the draws), mode,
    detail (the full record of draw `detail_at`, for a failure report))."""
    mode = sample_mode(case["top_k"], case["top_p"])
    inv_t = np.float32(1.0) if mode == GREEDY else inv_temp32(case["T"])      # top_k = 1 goes to the plain argmax: no temperature
    seen = None if seen0 is None else np.array(seen0, dtype=np.uint8)
    state = list(case["state"])
    n = case["n_draws"]
    toks, dec, dist, detail = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool), np.zeros(n), None
    min_margin, max_exp, surv_all = np.inf, 0.0, None
    cache = None
    for i in range(n):
        if cache is None or seen is not None:
            sc = processed(logits, seen, case["penalty"], case["suppress"], inv_t)
            surv = None if mode == GREEDY else survivors_of(mode, sc, case["top_k"], case["top_p"])
            cache = (sc, surv)
        sc, surv = cache
        r = expected(mode, sc, case["top_k"], case["top_p"], case["seed"], state[1] + 1, surv)
        if surv is not None:
            min_margin = min(min_margin, surv[1])
            max_exp = max(max_exp, surv[2]["exp_err"])
            surv_all = surv[0].copy() if surv_all is None else (surv_all | surv[0])
        toks[i], dec[i], dist[i] = r["token"], r["decided"], r["dist"]
        if detail_at == i:
            detail = r
        t = int(gpu_tokens[i]) if gpu_tokens is not None else r["token"]
        if seen is not None:
            seen[t] = 1
        state[1] += 1
        state[0] += case["advance_kv"]
    return dict(tokens=toks, decided=dec, dist=dist, detail=detail, seen=seen, state=state, min_margin=min_margin, max_exp_err=max_exp,
                survivors=surv_all, mode=mode)
