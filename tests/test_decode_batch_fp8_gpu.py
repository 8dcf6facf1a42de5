"""Lane-batched decode kernels on e4m3 weights (csrc/decode_batch_fp8.hip) through the C ABI.

The yardstick is the existing single-row fp8 kernel (csrc/decode_fp8.hip) run once per lane on copies of the same inputs, never the
batched code itself, and the bar is BITWISE equality: the batched kernels keep the single-row arithmetic order per (lane, output row),
so there is no tolerance.  Weights come from quantize_rows_fp8_pow2 with row magnitudes spread over decades, so the scales differ per
row.  Lanes get different inputs, norms, KV lengths, pools and slot tables; every pool and linear plane is pre-filled with a sentinel
pattern so that a row written anywhere but a lane's own new row shows.
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
    "3b": (2048, 11008, 16, 2),
}
# the form of svlm_gemv_fp8 (rows per wave, waves that share K) each residual GEMV must take, restated from its dispatch
GEMV_FORMS = {                  # name: (o_proj, down_proj)
    "tiny": ((1, 1), (1, 1)),
    "2b": ((1, 1), (2, 4)),
    "7b": ((2, 1), (2, 4)),
    "3b": ((1, 1), (2, 4)),
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


def q8(shape, seed, scale):
    """Random rows over two decades of magnitude (distinct power-of-two scales), quantised: (codes, scales) on the GPU."""
    from streaming_vlm_amd.weights import quantize_rows_fp8_pow2
    g = torch.Generator().manual_seed(seed + 1000)
    mag = 10.0 ** (torch.rand((shape[0], 1), generator=g) * 2 - 1)
    w = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale * mag).to(BF16)
    q, s = quantize_rows_fp8_pow2(w)
    assert len(torch.unique(s)) >= 4, "the rows must not share one scale"
    return q.cuda(), s.cuda()


def bits(t):
    return t.view(torch.int16) if t.dtype == BF16 else (t.view(torch.int32) if t.dtype == torch.float32 else t)


def same(name, got, want):
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ne = bits(got) != bits(want)
    assert not bool(ne.any()), f"{name}: {int(ne.sum())} of {ne.numel()} elements differ bitwise"


class Lane:
    """Everything one lane owns."""

    def __init__(self, b, Hkv, V, kv_len, cur, limit, penalty=1.05, n_suppress=2, seed=0):
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


def make_lanes(B, Hkv, V, dead=()):
    # different KV lengths and token counters per lane; a lane in `dead` has used up its limit (state[1] + 1 == limit)
    return [Lane(b, Hkv, V, kv_len=7 + 9 * b, cur=1 + b, limit=(2 + b) if b in dead else 10) for b in range(B)]


_W = {}


def weights(name):
    if name not in _W:
        H, I, hq, hkv = SHAPES[name]
        qd, kd = hq * D, hkv * D
        s = 1.0 / np.sqrt(H)
        _W[name] = dict(ln=rnd((H,), 1, 1.0), qkv=q8((qd + 2 * kd, H), 2, s), qkv_b=rnd((qd + 2 * kd,), 3, 0.5), o=q8((H, qd), 4, 1.0 / np.sqrt(qd)),
                        gu=q8((2 * I, H), 5, s), down=q8((H, I), 6, 1.0 / np.sqrt(I)))
    return _W[name]


def gemv_form(N, K):
    """(rows per wave, waves sharing K) of svlm_gemv_fp8 for an [N, K] matrix -- its dispatch, restated."""
    if N <= 8192 and K >= 4096:
        return (2, 4)
    if N >= 16384:
        return (4, 1)
    if N >= 4096 or N * K >= (8 << 20):
        return (2, 1)
    return (1, 1)


def test_residual_gemv_shapes_reach_the_plain_forms_and_the_k_split():
    """The widths below take both ROWS choices of the plain form (o_proj) and the KW = 4 long-K form (down_proj at 2B, 3B and 7B)."""
    forms = set()
    for name, (H, I, hq, _) in SHAPES.items():
        got = (gemv_form(H, hq * D), gemv_form(H, I))
        assert got == GEMV_FORMS[name], (name, got)
        forms.update(got)
    assert {(1, 1), (2, 1), (2, 4)} <= forms


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_layer_kernels_bitwise_equal_single_row_fp8(ops, name, B):
    H, I, hq, hkv = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = weights(name)
    V = 1000
    lanes = make_lanes(B, hkv, V)
    tab = lane_table(ops, lanes)
    x = rnd((B, H), 10 + B, 1.0)
    for b in range(B):
        x[b] *= (b + 1) * 0.7                     # different norms per lane
    attn, hrow = rnd((B, qd), 20 + B), rnd((B, I), 30 + B)
    layer = 1
    # ---- yardstick: the single-row fp8 entries, lane by lane, on copies
    want = []
    for b, ln in enumerate(lanes):
        pool, lin = ln.pool.clone(), ln.lin.clone()
        q = torch.zeros(qd, dtype=BF16).cuda()
        ops.dec_qkv_fp8(x[b], w["ln"], 1e-6, *w["qkv"], w["qkv_b"], q, pool, layer, ln.slot_of, qd, kd, len_dev=ln.state[0:1], lin=(lin, ln.lin_len))
        xo = x[b].clone()
        ops.gemv_fp8(attn[b], *w["o"], residual=xo, out=xo)
        h = torch.zeros(I, dtype=BF16).cuda()
        ops.dec_gate_up_fp8(x[b], w["ln"], 1e-6, *w["gu"], h)
        xd = x[b].clone()
        ops.gemv_fp8(hrow[b], *w["down"], residual=xd, out=xd)
        want.append(dict(q=q, pool=pool, lin=lin, xo=xo, h=h, xd=xd))
    # ---- batched
    before = [ln.snapshot() for ln in lanes]
    q = torch.zeros((B, qd + 2 * kd), dtype=BF16).cuda()                  # (a group's q|k|v-wide buffer: the row stride is not qd)
    ops.decb_qkv_fp8(tab, B, x, w["ln"], 1e-6, *w["qkv"], w["qkv_b"], q, layer, qd, kd, D, N_LAYERS)
    xo = x.clone()
    ops.decb_gemv_fp8(tab, B, attn, *w["o"], xo, xo)
    h = torch.zeros((B, I), dtype=BF16).cuda()
    ops.decb_gate_up_fp8(tab, B, x, w["ln"], 1e-6, *w["gu"], h)
    xd = x.clone()
    ops.decb_gemv_fp8(tab, B, hrow, *w["down"], xd, xd)
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
    assert bool((q[:, qd:] == 0).all()), "q_out written past the q columns"


@pytest.mark.parametrize("B", [2, 4])
def test_residual_gemv_tall_output_form_bitwise_equal_single_row_fp8(ops, B):
    """N >= 16384: the 4-rows-per-wave form of svlm_gemv_fp8, which no o_proj / down_proj width above reaches; N is not a multiple of
    the 16 rows of a workgroup."""
    N, K = 16384 + 6, 512
    assert gemv_form(N, K) == (4, 1)
    W = q8((N, K), 13, 1.0 / np.sqrt(K))
    lanes = make_lanes(B, 2, 100)
    tab = lane_table(ops, lanes)
    x, res = rnd((B, K), 50 + B), rnd((B, N), 60 + B)
    y = res.clone()
    ops.decb_gemv_fp8(tab, B, x, *W, y, y)
    for b in range(B):
        want = res[b].clone()
        ops.gemv_fp8(x[b], *W, residual=want, out=want)
        same(f"y[{b}]", y[b], want)


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("H,V", [(256, 151680), (1536, 151936)])
def test_lm_head_and_token_feedback_bitwise_equal_single_row_fp8(ops, H, V, B):
    W = q8((V, H), 7, 1.0 / np.sqrt(H))
    ln_w = rnd((H,), 8)
    lanes = make_lanes(B, 2, V)
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
            # the group has ONE suppress list: it holds lane 0's two would-be winners, so suppression decides lane 0's token; the other
            # suppressing lanes get the same ids (not their winners) and check that the list is applied per lane by n_suppress
            logits0 = torch.zeros(V, dtype=torch.float32).cuda()
            ops.dec_lm_head_fp8(x[b], ln_w, 1e-6, *W, logits0, None, 1.0, None, ops.sampling_ws(V, "cuda"))
            if b == 0:
                suppress[:2] = torch.topk(logits0, 2).indices.to(torch.int32)
            sup = suppress[:2]
        logits = torch.zeros(V, dtype=torch.float32).cuda()
        ws = ops.sampling_ws(V, "cuda")
        ws.zero_()
        seen, tok, st = ln.seen.clone(), ln.tok_buf.clone(), ln.state.clone()
        ops.dec_lm_head_fp8(x[b], ln_w, 1e-6, *W, logits, seen, ln.penalty, sup, ws)
        nb = (V + 7) // 8
        cand = ws[:2 * nb].clone()
        ops.argmax_finish(ws, V, seen, tok, st, 1)
        want.append(dict(logits=logits, cand=cand, seen=seen, tok=tok, st=st))
    logits = torch.zeros((B, V), dtype=torch.float32).cuda()
    ws = ops.decb_sampling_ws(V, B, "cuda")
    ws.zero_()
    ops.decb_lm_head_fp8(tab, B, x, ln_w, 1e-6, *W, logits, suppress, ws)
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


@pytest.mark.parametrize("name", ["tiny", "2b"])
def test_inactive_lane_is_untouched_by_a_full_batched_fp8_step(ops, name):
    """A lane whose state says it is past its limit: every kernel of a step skips it -- pool, linear planes, tok_buf, state, seen and
    its rows of the group buffers keep their bits -- while the live lanes compute what they compute without it."""
    H, I, hq, hkv = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = weights(name)
    V, B, dead = 3000, 3, 1
    table, head = rnd((V, H), 11), q8((V, H), 12, 1.0 / np.sqrt(H))
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
        ops.decb_qkv_fp8(tab, B, x, w["ln"], 1e-6, *w["qkv"], w["qkv_b"], q, 0, qd, kd, D, N_LAYERS)
        ops.decb_gemv_fp8(tab, B, q, *w["o"], x, x)
        ops.decb_gate_up_fp8(tab, B, x, w["ln"], 1e-6, *w["gu"], h)
        ops.decb_gemv_fp8(tab, B, h, *w["down"], x, x)
        ops.decb_lm_head_fp8(tab, B, x, w["ln"], 1e-6, *head, logits, suppress, ws)
        ops.decb_argmax_finish(tab, B, ws, V, 1)
        torch.cuda.synchronize()
        return dict(x=x, q=q, h=h, logits=logits, ws=ws)

    lanes = make_lanes(B, hkv, V, dead=(dead,))
    before = lanes[dead].snapshot()
    got = step(lanes, B)
    for k, v in lanes[dead].snapshot().items():
        same(f"inactive lane {k}", v, before[k])
    for k, fill in (("x", 0.25), ("q", 0.5), ("h", 0.75), ("logits", -1.0), ("ws", -2.0)):
        assert bool((got[k][dead] == fill).all()), f"inactive lane's row of {k} was written"
    # the live lanes: the same step without the inactive lane in the group
    alone = [ln for b, ln in enumerate(make_lanes(B, hkv, V, dead=(dead,))) if b != dead]
    ref = step(alone, B - 1)
    for i, b in enumerate(b for b in range(B) if b != dead):
        for k in ("x", "q", "h", "logits"):
            same(f"live lane {b} {k}", got[k][b], ref[k][i])
        for k, v in lanes[b].snapshot().items():
            same(f"live lane {b} {k}", v, alone[i].snapshot()[k])
        assert int(lanes[b].state[1]) == lanes[b].cur + 1


def test_bad_arguments_are_refused(ops):
    from streaming_vlm_amd import _lib
    from streaming_vlm_amd.ops import _ptr, _stream
    w = weights("tiny")
    lanes = make_lanes(2, 2, 100)
    tab = lane_table(ops, lanes)
    x = rnd((2, 256), 1)
    h5, h2 = torch.zeros((5, 512), dtype=BF16).cuda(), torch.zeros((2, 512), dtype=BF16).cuda()
    with pytest.raises(_lib.SvlmError):
        ops.decb_gate_up_fp8(tab, 5, x, w["ln"], 1e-6, *w["gu"], h5)                                  # B > 4 (wrapper)
    with pytest.raises(_lib.SvlmError):
        ops.decb_gate_up_fp8(tab, 2, x[:1], w["ln"], 1e-6, *w["gu"], h2)                              # too few x rows
    with pytest.raises(_lib.SvlmError):
        ops.decb_gemv_fp8(tab[:, :8].contiguous(), 2, x, *w["o"], x, x)                               # malformed lane table
    with pytest.raises(_lib.SvlmError):
        ops.decb_gemv_fp8(tab, 2, x, w["o"][0][:, :248], w["o"][1], x, x)                             # K not a multiple of 16 (wrapper)
    # the entry points' own checks, below the wrapper: B = 5, K % 16 != 0, null scales
    gu8, gus = w["gu"]
    o8, os_ = w["o"]
    lib = ops.lib

    def gate_up(B=2, K=256, scale=gus):
        return lib.svlm_decb_gate_up_fp8(_ptr(tab), B, _ptr(x), 256, _ptr(w["ln"]), 1e-6, _ptr(gu8), 256, _ptr(scale), _ptr(h5), 512, 512, K, _stream())

    def gemv(B=2, K=512, scale=os_):
        xa = torch.zeros((4, 512), dtype=BF16).cuda()
        return lib.svlm_decb_gemv_fp8(_ptr(tab), B, _ptr(xa), 512, _ptr(o8), 512, _ptr(scale), _ptr(x), 256, _ptr(x), 256, 256, K, _stream())

    for what, rc in (("gate_up B=5", gate_up(B=5)), ("gate_up K=248", gate_up(K=248)), ("gate_up null scales", gate_up(scale=None)),
                     ("gemv B=5", gemv(B=5)), ("gemv K=504", gemv(K=504)), ("gemv null scales", gemv(scale=None)),
                     ("qkv null scales", lib.svlm_decb_qkv_fp8(_ptr(tab), 2, _ptr(x), 256, _ptr(w["ln"]), 1e-6, _ptr(w["qkv"][0]), 256, None,
                                                               _ptr(w["qkv_b"]), _ptr(h2), 512, 0, 256, 512, 256, D, _stream())),
                     ("lm_head B=0", lib.svlm_decb_lm_head_fp8(_ptr(tab), 0, _ptr(x), 256, _ptr(w["ln"]), 1e-6, _ptr(gu8), 256, _ptr(gus),
                                                               _ptr(torch.zeros((2, 1024), dtype=torch.float32).cuda()), 1024, _ptr(tab), _ptr(tab),
                                                               1024, 256, _stream()))):
        assert rc != 0, f"{what}: accepted"
        with pytest.raises(_lib.SvlmError):
            ops._check(rc, what)
    torch.cuda.synchronize()
