"""Wide lane-batched decode kernels (csrc/decode_wide.hip: the weight GEMVs of a group's decode step on the MFMA, 1..16 lanes) through
the C ABI, on the Lane / sentinel-pool scheme of tests/test_decode_batch_gpu.py.

The wide kernels keep the staged (normalised) rows and every rounding point of the single-row kernels but sum the dot products in the
MFMA's order, so the yardsticks are
  1. the fp64 reference and per-element bound of tests/gemv_ref64.py with c = 32 + ceil(kps / 32) + splits + [bias] fp32 additions
     (tests/gemm_ref64.py's count for bf16 MFMA paths; kps and splits are read off the library's split plan, svlm_decw_plan), the fused
     entries against the fp64 GEMV of the kernel family's OWN staged row (recovered through the single-row head with W = I);
  2. bit equality with the single-row kernels on the `bits` operands of tests/gemv_paths.py (exact in fp32 in any order);
  3. the side effects of tests/test_decode_batch_gpu.py: K/V rows in the lane's own slot and nowhere else, dead lanes untouched, the
     token equal to the fp64 argmax wherever the fp64 top-2 margin exceeds twice the bound, state / tok_buf / seen advanced;
  4. lane independence: bitwise the same lane at B = 16, at B = 1, in another column, and beside a dead lane full of NaN;
  5. determinism; 6. refusals.
"""
import math

import numpy as np
import pytest
import torch

import gemv_paths as G
import gemv_ref64 as R

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 128
EPS = 1e-6
SHAPES = {                      # name: (hidden, intermediate, q heads, kv heads, vocabulary)
    "tiny": (256, 512, 4, 2, 2011),
    "ragged": (1056, 2080, 3, 1, 1000),           # 33 x 32 and 65 x 32: K-step and K-split tails; V ends inside a 16-row tile
    "2b": (1536, 8960, 12, 2, 151936),
    "7b": (3584, 18944, 28, 4, 3000),             # B = 16 stages 16 x 3592 x 2 = 112 KB
}
N_LAYERS = 2
LAYER = 1
SENTINEL = 0x7b7b
FILL = {"q": 0.5, "xo": 0.25, "h": 0.75, "xd": 0.125, "logits": -1.0, "ws": -2.0}


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def same(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ bitwise"


def grnd(shape, seed, scale=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return (torch.randn(shape, generator=g, device="cuda") * scale).to(BF16)


class Lane:
    """Everything one lane owns.  `ident` seeds it: the same ident is the same lane whatever column it is put in."""

    def __init__(self, ident, Hkv, V, dead=False):
        g = torch.Generator().manual_seed(1000 + 17 * ident)
        self.ident, self.dead = ident, dead
        self.n_slots = 64 + 16 * (ident % 5)
        self.max_len = 48 + 16 * (ident % 5)
        self.pool = torch.full((N_LAYERS, 2, Hkv, self.n_slots, D), SENTINEL, dtype=torch.int16).view(BF16).cuda()
        self.lin = torch.full((N_LAYERS, 2, Hkv, self.max_len, D), SENTINEL, dtype=torch.int16).view(BF16).cuda()
        self.slot_of = torch.randperm(self.n_slots, generator=g)[:self.max_len].to(torch.int32).cuda()
        self.kv_len, self.cur = 7 + 2 * ident, 1 + ident % 8
        self.limit = self.cur + 1 if dead else 11           # dead: state[1] + 1 == limit
        self.state = torch.tensor([self.kv_len, self.cur], dtype=torch.int32).cuda()
        self.tok_buf = torch.randint(0, V, (12,), generator=g).to(torch.int32).cuda()
        self.seen = (torch.rand(V, generator=g) < 0.3).to(torch.uint8).cuda()
        self.penalty = 1.05 + 0.05 * (ident % 4)
        self.n_suppress = 2 if ident % 2 == 0 else 0

    def record(self, ops):
        return ops.lane_record(self.pool, self.lin, self.slot_of, self.state, self.tok_buf, self.seen, self.limit, self.penalty, self.n_suppress)

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("pool", "lin", "state", "tok_buf", "seen")}


def lane_table(ops, lanes):
    return torch.from_numpy(np.stack([ln.record(ops) for ln in lanes])).cuda()


def dead_set(B):
    return (1, B - 2) if B >= 4 else ()


_W = {}


def weights(name):
    """bf16 weights of one layer + head on the GPU, with their exact float32 copies for the fp64 reference; one shape at a time."""
    if name not in _W:
        _W.clear()
        torch.cuda.empty_cache()
        H, I, hq, hkv, V = SHAPES[name]
        qd, kd = hq * D, hkv * D
        s = 1.0 / math.sqrt(H)
        w = dict(ln=(grnd((H,), 1, 0.3).float() + 1.0).to(BF16), qkv_w=grnd((qd + 2 * kd, H), 2, s), qkv_b=grnd((qd + 2 * kd,), 3, 0.5),
                 o_w=grnd((H, qd), 4, 1.0 / math.sqrt(qd)), gu_w=grnd((2 * I, H), 5, s), down_w=grnd((H, I), 6, 1.0 / math.sqrt(I)),
                 head=grnd((V, H), 7, s), embed=grnd((64, H), 8))
        _W[name] = w
    return _W[name]


def wf32(name, W):
    """The exact float32 copy of a weight matrix, kept with the shape's weights."""
    f = _W[name].setdefault("_f32", {})
    if W.data_ptr() not in f:
        f[W.data_ptr()] = W.float()
    return f[W.data_ptr()]


def inputs(name, idents):
    """Per-lane activation rows, seeded by the lane's ident (so a lane keeps its inputs when it changes column)."""
    H, I, hq, hkv, V = SHAPES[name]
    x = torch.stack([grnd((H,), 100 + i, 0.7 * (1 + i % 3)) for i in idents])
    attn = torch.stack([grnd((hq * D,), 200 + i) for i in idents])
    hrow = torch.stack([grnd((I,), 300 + i) for i in idents])
    return dict(x=x, attn=attn, hrow=hrow)


def suppress_ids(V):
    return torch.tensor([5, V - 3, 0, 0, 0, 0, 0, 0], dtype=torch.int32).cuda()


def wide_step(ops, name, lanes, inp, w=None):
    """Every wide entry once on the group's rows -> the group buffers (dead lanes' rows keep their fill)."""
    H, I, hq, hkv, V = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = w or weights(name)
    B = len(lanes)
    tab = lane_table(ops, lanes)
    x = inp["x"]
    q = torch.full((B, qd + 2 * kd), FILL["q"], dtype=BF16).cuda()           # (a q|k|v-wide buffer: the row stride is not qd)
    ops.decw_qkv(tab, B, x, w["ln"], EPS, w["qkv_w"], w["qkv_b"], q, LAYER, qd, kd, D, N_LAYERS)
    xo = x.clone()
    for b, ln in enumerate(lanes):
        if ln.dead:
            xo[b] = FILL["xo"]
    ops.decw_gemv(tab, B, inp["attn"], w["o_w"], xo, xo)
    h = torch.full((B, I), FILL["h"], dtype=BF16).cuda()
    ops.decw_gate_up(tab, B, x, w["ln"], EPS, w["gu_w"], h)
    xd = x.clone()
    for b, ln in enumerate(lanes):
        if ln.dead:
            xd[b] = FILL["xd"]
    ops.decw_gemv(tab, B, inp["hrow"], w["down_w"], xd, xd)
    logits = torch.full((B, V), FILL["logits"], dtype=torch.float32).cuda()
    ws = ops.decb_sampling_ws(V, B, "cuda")
    ws.fill_(FILL["ws"])
    ops.decw_lm_head(tab, B, x, w["ln"], EPS, w["head"], logits, suppress_ids(V), ws)
    cand = ws.clone()
    ops.decw_argmax_finish(tab, B, ws, V, 1)
    torch.cuda.synchronize()
    return dict(q=q, xo=xo, h=h, xd=xd, logits=logits, ws=cand)


def new_kv(ln, hkv):
    """The lane's new K and V rows of LAYER as one vector (K heads then V heads), read from its pool slot."""
    slot = int(ln.slot_of[ln.kv_len])
    return torch.cat([ln.pool[LAYER, 0, :, slot, :].reshape(-1), ln.pool[LAYER, 1, :, slot, :].reshape(-1)])


def lane_outputs(out, b, ln, qd, hkv):
    return dict(qkv=torch.cat([out["q"][b, :qd], new_kv(ln, hkv)]), xo=out["xo"][b], h=out["h"][b], xd=out["xd"][b], logits=out["logits"][b],
                pool=ln.pool, lin=ln.lin, state=ln.state, tok_buf=ln.tok_buf, seen=ln.seen)


_IDENT = {}


def staged_row(ops, x, gain):
    """xs of dec_xrow.h:stage_x, bit for bit, through the existing single-row head with W = I (tests/gemv_ref64.py)."""
    K = x.numel()
    if K not in _IDENT:
        _IDENT.clear()
        _IDENT[K] = torch.eye(K, dtype=BF16, device="cuda")
    logits = torch.zeros(K, dtype=torch.float32, device="cuda")
    ws = torch.empty(ops.lib.svlm_dec_lm_head_ws_bytes(K) // 4 + 1, dtype=torch.float32, device="cuda")
    ops.dec_lm_head(x, gain, EPS, _IDENT[K], logits, None, 1.0, None, ws)
    xs = logits.cpu()
    assert torch.equal(xs.to(BF16).float(), xs), "the staged row must be bf16 values"
    return xs.to(BF16)


def fadds(ops, fused, K, bias):
    splits, kps = ops.decw_plan(fused, K)
    return 32 + -(-kps // 32) + splits + (1 if bias else 0), splits, kps


CASES = [(n, B) for n in ("tiny", "ragged") for B in (1, 4, 5, 9, 16)] + [("2b", 9), ("7b", 16)]


@pytest.mark.parametrize("name,B", CASES, ids=[f"{n}-B{B}" for n, B in CASES])
def test_every_entry_against_fp64_bound_and_side_effects(ops, name, B):
    H, I, hq, hkv, V = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = weights(name)
    dead = dead_set(B)
    lanes = [Lane(b, hkv, V, dead=b in dead) for b in range(B)]
    inp = inputs(name, range(B))
    before = [ln.snapshot() for ln in lanes]
    out = wide_step(ops, name, lanes, inp)
    nb = (V + 7) // 8
    sup = suppress_ids(V).cpu()
    worst = {}
    for b, ln in enumerate(lanes):
        if ln.dead:
            for k, v in ln.snapshot().items():
                same(f"dead lane {b} {k}", v, before[b][k])
            for k in FILL:
                assert bool((out[k][b] == FILL[k]).all()), f"dead lane {b}: its row of {k} was written"
            continue
        xs = staged_row(ops, inp["x"][b], w["ln"])
        got = lane_outputs(out, b, ln, qd, hkv)
        checks = (("qkv", "qkv", w["qkv_w"], xs, True, w["qkv_b"], None, got["qkv"], H),
                  ("o_proj", "gemv", w["o_w"], inp["attn"][b], False, None, inp["x"][b], got["xo"], qd),
                  ("gate_up", "gate_up", w["gu_w"], xs, True, None, None, got["h"], H),
                  ("down_proj", "gemv", w["down_w"], inp["hrow"][b], False, None, inp["x"][b], got["xd"], I),
                  ("lm_head", "lm_head", w["head"], xs, True, None, None, got["logits"], H))
        for label, kind, W, xrow, fused, bias, res, y, K in checks:
            c, splits, kps = fadds(ops, fused, K, bias is not None)
            ref, bound = R.reference(kind, wf32(name, W), xrow, c, bias, res)
            ratio, mean = R.ratios(y.float(), ref, bound)
            wr = float(ratio.max())
            worst[label] = (max(worst.get(label, (0, 0))[0], wr), max(worst.get(label, (0, 0))[1], mean), c, splits, kps)
            assert torch.isfinite(y.float()).all() and wr <= 1.0 and mean <= R.MEAN_TOL, \
                f"{name} B={B} lane {b} {label}: worst err/bound {wr:.3f} mean {mean:.3f} (c={c}, {splits} splits of {kps})"
            if label == "lm_head":
                z, dz = ref, bound
        # ---- side effects: the lane's K/V in its own new slot and linear-plane row, everything else still the sentinel
        changed = (bits(ln.pool) != bits(before[b]["pool"])).any(dim=-1)
        expect = torch.zeros_like(changed)
        expect[LAYER, :, :, int(ln.slot_of[ln.kv_len])] = True
        assert torch.equal(changed, expect), f"lane {b}: pool rows written outside its own new row"
        lin_changed = bits(ln.lin) != bits(before[b]["lin"])
        assert int(lin_changed[LAYER].sum()) == 2 * hkv * D and not bool(lin_changed[1 - LAYER].any())
        kv = new_kv(ln, hkv)
        same(f"lin V[{b}]", ln.lin[LAYER, 1, :, ln.kv_len, :].reshape(-1), kv[kd:])
        krow = ln.lin[LAYER, 0].reshape(hkv, -1, 4, 4, 16, 8)[:, ln.kv_len >> 4, :, :, ln.kv_len & 15, :].reshape(-1)   # (h, d>>5, (d>>3)&3, d&7)
        same(f"lin K[{b}]", krow, kv[:kd])
        # ---- the token: the fp64 argmax of the penalised, suppressed scores wherever its top-2 margin exceeds twice the bound
        seen0 = before[b]["seen"].cpu().bool()
        pen = torch.where(seen0, torch.where(z < 0, torch.full_like(z, ln.penalty), torch.full_like(z, 1.0 / ln.penalty)), torch.ones_like(z))
        zs, ds = z * pen, dz * pen
        if ln.n_suppress:
            zs[sup[:ln.n_suppress].long()] = -math.inf
        top = torch.topk(zs, 2)
        tok = int(ln.tok_buf[ln.cur + 1])
        if float(top.values[0] - top.values[1]) > 2 * float(ds.max()):
            assert tok == int(top.indices[0]), f"lane {b}: token {tok}, fp64 argmax {int(top.indices[0])}"
        else:
            print(f"[decw] {name} B={B} lane {b}: fp64 top-2 margin within twice the bound, token not pinned")
        # the candidates: one per 8 vocabulary rows, each the best of ITS rows of the kernel's own scores
        lg = out["logits"][b].cpu()
        sc = torch.where(seen0, torch.where(lg < 0, lg * np.float32(ln.penalty), lg / np.float32(ln.penalty)), lg)
        if ln.n_suppress:
            sc[sup[:ln.n_suppress].long()] = -math.inf
        pad = torch.full((nb * 8,), -math.inf)
        pad[:V] = sc
        cv, ci = pad.view(nb, 8).max(dim=1)
        wsb = out["ws"][b].cpu()
        # (the host's fp32 division may differ from the device's in the last bit: one ulp of slack on the penalised values)
        assert torch.allclose(wsb[:nb], cv, rtol=2.5e-7, atol=0), f"lane {b}: candidate values"
        got_i = wsb[nb:2 * nb].view(torch.int32)
        assert torch.allclose(pad[got_i.long()], cv, rtol=2.5e-7, atol=0) and bool((got_i // 8 == torch.arange(nb)).all()), f"lane {b}: candidate indices"
        assert float(sc[tok]) >= float(sc.max()) - 2.5e-7 * abs(float(sc.max())), f"lane {b}: token {tok} is not the best of the kernel's own scores"
        # state / tok_buf / seen advance as decb_argmax_finish advances them
        assert ln.state.tolist() == [ln.kv_len + 1, ln.cur + 1]
        tb = before[b]["tok_buf"].clone()
        tb[ln.cur + 1] = tok
        same(f"tok_buf[{b}]", ln.tok_buf, tb)
        sn = before[b]["seen"].clone()
        sn[tok] = 1
        same(f"seen[{b}]", ln.seen, sn)
    for label, (wr, mean, c, splits, kps) in worst.items():
        print(f"[decw] {name} B={B} {label}: worst err/bound {wr:.3f} mean {mean:.3f} (c={c}: {splits} splits of {kps})")


@pytest.mark.parametrize("name,B", [("tiny", 16), ("ragged", 9)])
def test_exact_operands_are_bitwise_the_single_row_kernels(ops, name, B):
    """`bits` weights and +-1 probes (gain 1 stages x itself): every sum is exact in fp32 in any order, so the MFMA order does not show."""
    H, I, hq, hkv, V = SHAPES[name]
    qd, kd = hq * D, hkv * D
    n = torch.arange(4096)
    w = dict(ln=torch.ones(H, dtype=BF16).cuda(), qkv_w=G.weights("bf16", "bits", qd + 2 * kd, H, device="cuda")["W"],
             qkv_b=(n[:qd + 2 * kd] % 5 - 2).to(BF16).cuda(), o_w=G.weights("bf16", "bits", H, qd, device="cuda")["W"],
             gu_w=G.weights("bf16", "bits", 2 * I, H, device="cuda")["W"], down_w=G.weights("bf16", "bits", H, I, device="cuda")["W"],
             head=G.weights("bf16", "bits", V, H, device="cuda")["W"])

    def probes(K):
        p = G.bits_probes(K)
        return torch.stack([p[b % len(p)] * (1 if b < len(p) else -1) for b in range(B)]).cuda()

    lanes = [Lane(b, hkv, V, dead=b in dead_set(B)) for b in range(B)]
    inp = dict(x=probes(H), attn=probes(qd), hrow=probes(I))
    before = [ln.snapshot() for ln in lanes]
    out = wide_step(ops, name, lanes, inp, w)
    for b, ln in enumerate(lanes):
        if ln.dead:
            continue
        pool, lin = before[b]["pool"].clone(), before[b]["lin"].clone()
        q = torch.zeros(qd, dtype=BF16).cuda()
        lin_len = torch.tensor([ln.kv_len, 1], dtype=torch.int32).cuda()
        ops.dec_qkv(inp["x"][b], w["ln"], EPS, w["qkv_w"], w["qkv_b"], q, pool, LAYER, ln.slot_of, qd, kd, len_dev=before[b]["state"][0:1],
                    lin=(lin, lin_len))
        xo = inp["x"][b].clone()
        ops.gemv(inp["attn"][b], w["o_w"], residual=xo, out=xo)
        h = torch.zeros(I, dtype=BF16).cuda()
        ops.dec_gate_up(inp["x"][b], w["ln"], EPS, w["gu_w"], h)
        xd = inp["x"][b].clone()
        ops.gemv(inp["hrow"][b], w["down_w"], residual=xd, out=xd)
        logits = torch.zeros(V, dtype=torch.float32).cuda()
        ops.dec_lm_head(inp["x"][b], w["ln"], EPS, w["head"], logits, None, 1.0, None, ops.sampling_ws(V, "cuda"))
        same(f"q[{b}]", out["q"][b, :qd], q)
        same(f"pool[{b}]", ln.pool, pool)
        same(f"lin[{b}]", ln.lin, lin)
        same(f"o_proj[{b}]", out["xo"][b], xo)
        same(f"h[{b}]", out["h"][b], h)
        same(f"down_proj[{b}]", out["xd"][b], xd)
        same(f"logits[{b}]", out["logits"][b], logits)


@pytest.mark.parametrize("name", ["tiny", "ragged", "7b"])
def test_staged_rows_are_bitwise_the_single_row_prologue(ops, name):
    """W = I through decw_lm_head writes logits[n] = xs[n] (one product per sum): every lane's staged row against stage_x's, at 16
    lanes (each wave of the wide prologue stages four rows)."""
    H = SHAPES[name][0]
    B = 16
    lanes = [Lane(b, 1, H, dead=b in dead_set(B)) for b in range(B)]
    tab = lane_table(ops, lanes)
    x = inputs(name, range(B))["x"]
    gain = weights(name)["ln"]
    logits = torch.zeros((B, H), dtype=torch.float32).cuda()
    ws = ops.decb_sampling_ws(H, B, "cuda")
    staged_row(ops, x[0], gain)
    ops.decw_lm_head(tab, B, x, gain, EPS, _IDENT[H], logits, suppress_ids(H), ws)
    torch.cuda.synchronize()
    for b, ln in enumerate(lanes):
        if not ln.dead:
            same(f"{name} staged row of lane {b}", logits[b].cpu().to(BF16), staged_row(ops, x[b], gain))


@pytest.mark.parametrize("name", ["tiny", "ragged"])
def test_lane_independence_and_determinism(ops, name):
    H, I, hq, hkv, V = SHAPES[name]
    qd = hq * D
    B = 16
    dead = dead_set(B)

    def run(idents, poison=False):
        lanes = [Lane(i, hkv, V, dead=i in dead) for i in idents]
        inp = inputs(name, idents)
        if poison:
            for col, i in enumerate(idents):
                if i in dead:
                    for k in inp:
                        inp[k][col] = float("nan")
        out = wide_step(ops, name, lanes, inp)
        return {i: lane_outputs(out, col, lanes[col], qd, hkv) for col, i in enumerate(idents) if i not in dead}

    base = run(list(range(B)))
    again = run(list(range(B)))                                   # determinism: the same inputs, bit for bit
    moved = run(list(reversed(range(B))))                         # every lane in another column
    poisoned = run(list(range(B)), poison=True)                   # the dead lanes' activation rows full of NaN
    for i, want in base.items():
        for other, what in ((again, "second run"), (moved, "moved to another column"), (poisoned, "beside NaN rows of dead lanes")):
            for k, v in want.items():
                same(f"lane {i} {k} ({what})", other[i][k], v)
    for i in (0, 7, 15):                                          # the same lane alone: B = 1
        alone = run([i])
        for k, v in base[i].items():
            same(f"lane {i} {k} (B = 1)", alone[i][k], v)


def test_embed_accepts_16_lanes(ops):
    H, V, B = 1056, 64, 16
    table = weights("ragged")["embed"]
    lanes = [Lane(b, 1, V, dead=b in dead_set(B)) for b in range(B)]
    tab = lane_table(ops, lanes)
    x = torch.full((B, H), 0.25, dtype=BF16).cuda()
    ops.decw_embed(tab, B, table, x)
    torch.cuda.synchronize()
    for b, ln in enumerate(lanes):
        want = torch.full((H,), 0.25, dtype=BF16).cuda() if ln.dead else table[int(ln.tok_buf[ln.cur])]
        same(f"x[{b}]", x[b], want)


def test_bad_arguments_are_refused_without_a_launch(ops):
    from streaming_vlm_amd import _lib
    w = weights("tiny")
    H, I, hq, hkv, V = SHAPES["tiny"]
    lanes = [Lane(b, hkv, V) for b in range(2)]
    tab16 = torch.zeros((17, ops.LANE_WORDS), dtype=torch.int64).cuda()
    tab16[:2] = lane_table(ops, lanes)
    x, a = grnd((17, H), 1), grnd((17, hq * D), 2)
    x0 = x.clone()
    h = torch.full((17, I), 0.75, dtype=BF16).cuda()
    lib = ops.lib
    p = lambda t: t.data_ptr()
    # the C entries themselves (the Python wrappers check the same things first)
    for B in (0, 17):
        assert lib.svlm_decw_gate_up(p(tab16), B, p(x), H, p(w["ln"]), EPS, p(w["gu_w"]), H, p(h), I, I, H, None) != 0
        assert lib.svlm_decw_gemv(p(tab16), B, p(a), hq * D, p(w["o_w"]), hq * D, p(x), H, p(x), H, H, hq * D, None) != 0
        assert lib.svlm_decw_embed(p(tab16), B, p(w["embed"]), 64, p(x), H, H, None) != 0
        assert lib.svlm_decw_argmax_finish(p(tab16), B, p(h), V, 1, None) != 0
        with pytest.raises(_lib.SvlmError):
            ops.decw_gate_up(tab16, B, x, w["ln"], EPS, w["gu_w"], h)
    assert lib.svlm_decw_gate_up(p(tab16), 2, p(x), H, p(w["ln"]), EPS, p(w["gu_w"]), H, p(h), I, I, H - 4, None) != 0          # K % 8
    assert lib.svlm_decw_gemv(p(tab16), 2, p(a), hq * D, p(w["o_w"]), hq * D, p(x), H, p(x), H, H, hq * D - 4, None) != 0       # K % 8
    assert lib.svlm_decw_gate_up(p(tab16), 16, p(x), 4096, p(w["ln"]), EPS, p(w["gu_w"]), 4096, p(h), I, I, 4096, None) != 0    # 16 x 4104 x 2 B of LDS
    assert lib.svlm_decw_qkv(p(tab16), 1, p(x), 8192, p(w["ln"]), EPS, p(w["gu_w"]), 8192, p(h), p(h), 512, 0, 8192, 512, 256, D, None) != 0   # K > 4096
    assert lib.svlm_decw_gate_up(None, 2, p(x), H, p(w["ln"]), EPS, p(w["gu_w"]), H, p(h), I, I, H, None) != 0                   # no lane table
    with pytest.raises(_lib.SvlmError):
        ops.decw_gemv(tab16[:, :8].contiguous(), 2, x, w["o_w"], x, x)                                                            # malformed lane table
    with pytest.raises(_lib.SvlmError):
        ops.decw_gate_up(tab16, 2, x[:1], w["ln"], EPS, w["gu_w"], h)                                                             # too few x rows
    torch.cuda.synchronize()
    assert bool((h == 0.75).all()) and torch.equal(bits(x), bits(x0)), "a refused call launched"
