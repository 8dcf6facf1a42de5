"""Lane-batched decode kernels (csrc/decode_batch.hip) through the C ABI.

The yardstick is the existing single-row kernel run once per lane on the same inputs, never the batched code itself, and the
bar is BITWISE equality: the batched kernels keep the single-row arithmetic order per (lane, output row), so there is no tolerance.
Lanes get different inputs, KV lengths, pools and slot tables; every pool is pre-filled with a sentinel pattern so that a row
written anywhere but a lane's own new row shows.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 128
SHAPES = {                      # name: (hidden, intermediate, q heads, kv heads)
    "tiny": (256, 512, 4, 2),
    "2b": (1536, 8960, 12, 2),
    "7b": (3584, 18944, 28, 4),
}
N_LAYERS = 2
SENTINEL = 0x7b7b              # a finite bf16 bit pattern no kernel output here takes by accident in a whole row


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16).cuda()


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def same(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ bitwise"


class Lane:
    """Everything one lane owns, with a frozen copy for the single-row yardstick to work on."""

    def __init__(self, ops, b, Hkv, V, kv_len, cur, limit, penalty=1.05, n_suppress=2, seed=0):
        g = torch.Generator().manual_seed(1000 + 17 * b + seed)
        self.n_slots = 64 + 16 * b
        self.max_len = 48 + 16 * b
        self.pool = torch.full((N_LAYERS, 2, Hkv, self.n_slots, D), SENTINEL, dtype=torch.int16).view(BF16).cuda()
        self.lin = torch.full((N_LAYERS, 2, Hkv, self.max_len, D), SENTINEL, dtype=torch.int16).view(BF16).cuda()
        self.slot_of = torch.randperm(self.n_slots, generator=g)[:self.max_len].to(torch.int32).cuda()
        self.state = torch.tensor([kv_len, cur], dtype=torch.int32).cuda()
        self.tok_buf = torch.randint(0, V, (12,), generator=g).to(torch.int32).cuda()
        self.seen = (torch.rand(V, generator=g) < 0.3).to(torch.uint8).cuda()
        self.lin_len = torch.tensor([kv_len, 1], dtype=torch.int32).cuda()
        self.limit, self.penalty, self.n_suppress = limit, penalty, n_suppress
        self.kv_len, self.cur = kv_len, cur

    def record(self, ops):
        return ops.lane_record(self.pool, self.lin, self.slot_of, self.state, self.tok_buf, self.seen, self.limit, self.penalty, self.n_suppress)

    def snapshot(self):
        return {k: getattr(self, k).clone() for k in ("pool", "lin", "state", "tok_buf", "seen")}


def lane_table(ops, lanes):
    return torch.from_numpy(np.stack([ln.record(ops) for ln in lanes])).cuda()


def make_lanes(ops, B, Hkv, V, dead=()):
    # different KV lengths and token counters per lane; a lane in `dead` has used up its limit (state[1] + 1 == limit)
    return [Lane(ops, b, Hkv, V, kv_len=7 + 9 * b, cur=1 + b, limit=(2 + b) if b in dead else 10) for b in range(B)]


_W = {}


def weights(name):
    if name not in _W:
        H, I, hq, hkv = SHAPES[name]
        qd, kd = hq * D, hkv * D
        s = 1.0 / np.sqrt(H)
        _W[name] = dict(ln=rnd((H,), 1, 1.0), qkv_w=rnd((qd + 2 * kd, H), 2, s), qkv_b=rnd((qd + 2 * kd,), 3, 0.5), o_w=rnd((H, qd), 4, 1.0 / np.sqrt(qd)),
                        gu_w=rnd((2 * I, H), 5, s), down_w=rnd((H, I), 6, 1.0 / np.sqrt(I)))
    return _W[name]


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_layer_kernels_bitwise_equal_single_row(ops, name, B):
    H, I, hq, hkv = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = weights(name)
    V = 1000
    lanes = make_lanes(ops, B, hkv, V)
    tab = lane_table(ops, lanes)
    x = rnd((B, H), 10 + B, 1.0)
    for b in range(B):
        x[b] *= (b + 1) * 0.7                     # different norms per lane
    attn, hrow = rnd((B, qd), 20 + B), rnd((B, I), 30 + B)
    layer = 1
    # ---- yardstick: the single-row entries, lane by lane, on copies
    want = []
    for b, ln in enumerate(lanes):
        pool, lin = ln.pool.clone(), ln.lin.clone()
        q = torch.zeros(qd, dtype=BF16).cuda()
        ops.dec_qkv(x[b], w["ln"], 1e-6, w["qkv_w"], w["qkv_b"], q, pool, layer, ln.slot_of, qd, kd, len_dev=ln.state[0:1], lin=(lin, ln.lin_len))
        xo = x[b].clone()
        ops.gemv(attn[b], w["o_w"], residual=xo, out=xo)
        h = torch.zeros(I, dtype=BF16).cuda()
        ops.dec_gate_up(x[b], w["ln"], 1e-6, w["gu_w"], h)
        xd = x[b].clone()
        ops.gemv(hrow[b], w["down_w"], residual=xd, out=xd)
        want.append(dict(q=q, pool=pool, lin=lin, xo=xo, h=h, xd=xd))
    # ---- batched
    before = [ln.snapshot() for ln in lanes]
    q = torch.zeros((B, qd + 2 * kd), dtype=BF16).cuda()                  # (a group's q|k|v-wide buffer: the row stride is not qd)
    ops.decb_qkv(tab, B, x, w["ln"], 1e-6, w["qkv_w"], w["qkv_b"], q, layer, qd, kd, D, N_LAYERS)
    xo = x.clone()
    ops.decb_gemv(tab, B, attn, w["o_w"], xo, xo)
    h = torch.zeros((B, I), dtype=BF16).cuda()
    ops.decb_gate_up(tab, B, x, w["ln"], 1e-6, w["gu_w"], h)
    xd = x.clone()
    ops.decb_gemv(tab, B, hrow, w["down_w"], xd, xd)
    torch.cuda.synchronize()
    for b, ln in enumerate(lanes):
        same(f"q[{b}]", q[b, :qd], want[b]["q"])
        same(f"pool[{b}]", ln.pool, want[b]["pool"])
        same(f"lin[{b}]", ln.lin, want[b]["lin"])
        same(f"o_proj[{b}]", xo[b], want[b]["xo"])
        same(f"h[{b}]", h[b], want[b]["h"])
        same(f"down_proj[{b}]", xd[b], want[b]["xd"])
        # isolation: the pool differs from the sentinel fill in exactly the lane's own new row (both planes, every kv head) of `layer`
        changed = (bits(ln.pool) != bits(before[b]["pool"])).any(dim=-1)          # (layers, 2, Hkv, n_slots)
        expect = torch.zeros_like(changed)
        expect[layer, :, :, int(ln.slot_of[ln.kv_len])] = True
        assert torch.equal(changed, expect), f"lane {b}: pool rows written outside its own new row"
        lin_changed = bits(ln.lin) != bits(before[b]["lin"])
        assert int(lin_changed[layer].sum()) == 2 * hkv * D and not bool(lin_changed[1 - layer].any())
        same(f"state[{b}]", ln.state, before[b]["state"])


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("H,V", [(256, 151680), (1536, 151936)])
def test_lm_head_and_token_feedback_bitwise_equal_single_row(ops, H, V, B):
    W = rnd((V, H), 7, 1.0 / np.sqrt(H))
    ln_w = rnd((H,), 8)
    lanes = make_lanes(ops, B, 2, V)
    for b, ln in enumerate(lanes):
        ln.n_suppress = 2 if b % 2 == 0 else 0       # EOS suppressed on some lanes only
        ln.penalty = 1.05 + 0.1 * b
    tab = lane_table(ops, lanes)
    x = rnd((B, H), 40 + B, 2.0)
    suppress = torch.zeros(8, dtype=torch.int32).cuda()
    want = []
    for b, ln in enumerate(lanes):
        sup = None
        if ln.n_suppress:
            # make the suppressed ids the lane's would-be winners, so that suppression decides the token
            logits0 = torch.zeros(V, dtype=torch.float32).cuda()
            ops.dec_lm_head(x[b], ln_w, 1e-6, W, logits0, None, 1.0, None, ops.sampling_ws(V, "cuda"))
            if b == 0:
                suppress[:2] = torch.topk(logits0, 2).indices.to(torch.int32)
            sup = suppress[:2]
        logits = torch.zeros(V, dtype=torch.float32).cuda()
        ws = ops.sampling_ws(V, "cuda")
        ws.zero_()
        seen, tok, st = ln.seen.clone(), ln.tok_buf.clone(), ln.state.clone()
        ops.dec_lm_head(x[b], ln_w, 1e-6, W, logits, seen, ln.penalty, sup, ws)
        nb = (V + 7) // 8
        cand = ws[:2 * nb].clone()
        ops.argmax_finish(ws, V, seen, tok, st, 1)
        want.append(dict(logits=logits, cand=cand, seen=seen, tok=tok, st=st))
    logits = torch.zeros((B, V), dtype=torch.float32).cuda()
    ws = ops.decb_sampling_ws(V, B, "cuda")
    ws.zero_()
    ops.decb_lm_head(tab, B, x, ln_w, 1e-6, W, logits, suppress, ws)
    ops.decb_argmax_finish(tab, B, ws, V, 1)
    torch.cuda.synchronize()
    nb = (V + 7) // 8
    for b, ln in enumerate(lanes):
        same(f"logits[{b}]", logits[b], want[b]["logits"])
        same(f"candidates[{b}]", ws[b, :2 * nb], want[b]["cand"])
        same(f"tok_buf[{b}]", ln.tok_buf, want[b]["tok"])
        same(f"state[{b}]", ln.state, want[b]["st"])
        same(f"seen[{b}]", ln.seen, want[b]["seen"])
        assert int(ln.state[1]) == ln.cur + 1 and int(ln.state[0]) == ln.kv_len + 1


def test_embed_equals_gather_rows(ops):
    H, V, B = 1536, 5000, 4
    table = rnd((V, H), 9)
    lanes = make_lanes(ops, B, 2, V)
    tab = lane_table(ops, lanes)
    x = torch.zeros((B, H), dtype=BF16).cuda()
    ops.decb_embed(tab, B, table, x)
    for b, ln in enumerate(lanes):
        want = torch.zeros((1, H), dtype=BF16).cuda()
        ops.gather_rows(table, None, ln.tok_buf, want, idx_off=ln.state[1:2])
        same(f"x[{b}]", x[b], want[0])


@pytest.mark.parametrize("name", ["tiny", "2b"])
def test_inactive_lane_is_untouched_by_a_full_batched_step(ops, name):
    """A lane whose state says it is past its limit: every kernel of a step skips it -- pool, linear planes, tok_buf, state, seen and
    its rows of the group buffers keep their bits -- while the live lanes compute what they compute without it."""
    H, I, hq, hkv = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = weights(name)
    V, B, dead = 3000, 3, 1
    table, head = rnd((V, H), 11), rnd((V, H), 12, 1.0 / np.sqrt(H))
    suppress = torch.zeros(8, dtype=torch.int32).cuda()

    def step(lanes, B):
        tab = lane_table(ops, lanes)
        x = torch.full((B, H), 0.25, dtype=BF16).cuda()
        q = torch.full((B, qd), 0.5, dtype=BF16).cuda()
        h = torch.full((B, I), 0.75, dtype=BF16).cuda()
        logits = torch.full((B, V), -1.0, dtype=torch.float32).cuda()
        ws = ops.decb_sampling_ws(V, B, "cuda")
        ws.fill_(-2.0)
        ops.decb_embed(tab, B, table, x)
        ops.decb_qkv(tab, B, x, w["ln"], 1e-6, w["qkv_w"], w["qkv_b"], q, 0, qd, kd, D, N_LAYERS)
        ops.decb_gemv(tab, B, q, w["o_w"], x, x)
        ops.decb_gate_up(tab, B, x, w["ln"], 1e-6, w["gu_w"], h)
        ops.decb_gemv(tab, B, h, w["down_w"], x, x)
        ops.decb_lm_head(tab, B, x, w["ln"], 1e-6, head, logits, suppress, ws)
        ops.decb_argmax_finish(tab, B, ws, V, 1)
        torch.cuda.synchronize()
        return dict(x=x, q=q, h=h, logits=logits, ws=ws)

    lanes = make_lanes(ops, B, hkv, V, dead=(dead,))
    before = lanes[dead].snapshot()
    got = step(lanes, B)
    for k, v in lanes[dead].snapshot().items():
        same(f"inactive lane {k}", v, before[k])
    for k, fill in (("x", 0.25), ("q", 0.5), ("h", 0.75), ("logits", -1.0), ("ws", -2.0)):
        assert bool((got[k][dead] == fill).all()), f"inactive lane's row of {k} was written"
    # the live lanes: the same step without the inactive lane in the group
    alone = [ln for b, ln in enumerate(make_lanes(ops, B, hkv, V, dead=(dead,))) if b != dead]
    ref = step(alone, B - 1)
    for i, b in enumerate(b for b in range(B) if b != dead):
        for k in ("x", "q", "h", "logits"):
            same(f"live lane {b} {k}", got[k][b], ref[k][i])
        for k, v in lanes[b].snapshot().items():
            same(f"live lane {b} {k}", v, alone[i].snapshot()[k])
        assert int(lanes[b].state[1]) == lanes[b].cur + 1


def test_bad_arguments_are_refused(ops):
    from streaming_vlm_amd import _lib
    w = weights("tiny")
    lanes = make_lanes(ops, 2, 2, 100)
    tab = lane_table(ops, lanes)
    x = rnd((2, 256), 1)
    with pytest.raises(_lib.SvlmError):
        ops.decb_gate_up(tab, 5, x, w["ln"], 1e-6, w["gu_w"], torch.zeros((5, 512), dtype=BF16).cuda())          # B > 4
    with pytest.raises(_lib.SvlmError):
        ops.decb_gate_up(tab, 2, x[:1], w["ln"], 1e-6, w["gu_w"], torch.zeros((2, 512), dtype=BF16).cuda())       # too few x rows
    with pytest.raises(_lib.SvlmError):
        ops.decb_gemv(tab[:, :8].contiguous(), 2, x, w["o_w"][:, :256].contiguous(), x, x)                           # malformed lane table
