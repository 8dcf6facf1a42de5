"""Lane-batched decode kernels on MXFP4 weights (csrc/decode_batch_fp4.hip) through the C ABI.

The yardstick is the existing single-row fp4 kernel (csrc/decode_fp4.hip: dec_qkv_fp4, dec_gate_up_fp4, gemv_fp4, themselves held to an
fp64 per-element bound by tests/test_gemv_paths_gpu.py) run once per lane on copies of the same inputs, never the batched code itself,
and the bar is BITWISE equality: the batched kernels keep the single-row arithmetic order per (lane, output row), so there is no
tolerance.  Weights come from quantize_blocks_mxfp4 on rows whose magnitudes are spread over two decades; every matrix must carry at
least 4 distinct scale bytes and at least one row whose blocks carry more than one (a kernel that applied one scale per row could not
pass).  Lanes get different inputs, norms, KV lengths, pools and slot tables; every pool and linear plane is pre-filled with a sentinel
pattern so that a row written anywhere but a lane's own new row shows.
"""
import numpy as np
import pytest
import torch

from test_decode_batch_fp8_gpu import BF16, D, N_LAYERS, bits, lane_table, make_lanes, rnd, same

pytestmark = pytest.mark.gpu

SHAPES = {                      # name: (hidden, intermediate, q heads, kv heads)
    "tiny": (256, 512, 4, 2),
    "2b": (1536, 8960, 12, 2),
    "3b": (2048, 11008, 16, 2),
    "7b": (3584, 18944, 28, 4),
}
# the form of svlm_gemv_fp4 each residual GEMV must take, restated from its dispatch: (rows per wave, waves that share K, K-steps of
# 2048 the longest wave share takes)
GEMV_FORMS = {                  # name: (o_proj, down_proj)
    "tiny": ((1, 1, 1), (1, 1, 1)),
    "2b": ((1, 1, 1), (2, 4, 2)),          # kq = 2240
    "3b": ((1, 1, 1), (2, 4, 2)),          # kq = 2752
    "7b": ((2, 1, 2), (2, 4, 3)),          # kq = 4736: two iterations of the single-row kernel's PRE = 2 loop, the second ragged
}


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def q4(shape, seed, scale):
    """Random rows over two decades of magnitude, quantised to MXFP4: (codes [N, K / 2], e8m0 scales [N, K / 32]) on the GPU."""
    from streaming_vlm_amd.weights import quantize_blocks_mxfp4
    g = torch.Generator().manual_seed(seed + 1000)
    mag = 10.0 ** (torch.rand((shape[0], 1), generator=g) * 2 - 1)
    w = (torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale * mag).to(BF16)
    q, s = quantize_blocks_mxfp4(w)
    assert len(torch.unique(s)) >= 4, "the matrix must carry at least 4 distinct scale bytes"
    assert bool((s.min(dim=1).values != s.max(dim=1).values).any()), "some row must carry more than one scale byte"
    return q.cuda(), s.cuda()


_W = {}


def weights(name):
    if name not in _W:
        H, I, hq, hkv = SHAPES[name]
        qd, kd = hq * D, hkv * D
        s = 1.0 / np.sqrt(H)
        _W[name] = dict(ln=rnd((H,), 1, 1.0), qkv=q4((qd + 2 * kd, H), 2, s), qkv_b=rnd((qd + 2 * kd,), 3, 0.5), o=q4((H, qd), 4, 1.0 / np.sqrt(qd)),
                        gu=q4((2 * I, H), 5, s), down=q4((H, I), 6, 1.0 / np.sqrt(I)))
    return _W[name]


def gemv_form(N, K):
    """(rows per wave, waves sharing K, K-steps of the longest share) of svlm_gemv_fp4 for an [N, K] matrix -- its dispatch, restated."""
    if N <= 8192 and K >= 4096:
        kq = ((K // 32 + 3) // 4) * 32
        return (2, 4, (kq + 2047) // 2048)
    if N >= 4096 or N * K >= (8 << 20):
        return (2, 1, (K + 2047) // 2048)
    return (1, 1, (K + 2047) // 2048)


def fused_form(K):
    """<PRE, XC> of the fused kernels (DEC4_DISPATCH of decode_fp4.hip)."""
    return (1, 1) if K <= 2048 else ((2, 2) if K <= 4096 else (2, 4))


def test_shapes_reach_the_forms_they_are_here_for():
    forms = set()
    for name, (H, I, hq, _) in SHAPES.items():
        got = (gemv_form(H, hq * D), gemv_form(H, I))
        assert got == GEMV_FORMS[name], (name, got)
        forms.update(got)
    assert {(1, 1, 1), (2, 1, 2), (2, 4, 2), (2, 4, 3)} <= forms
    assert [((I // 32 + 3) // 4) * 32 for _, I, _, _ in (SHAPES["2b"], SHAPES["3b"], SHAPES["7b"])] == [2240, 2752, 4736]
    assert {fused_form(SHAPES[n][0]) for n in SHAPES} == {(1, 1), (2, 2)}
    assert [gemv_form(N, K) for N, K in EXTRA_GEMV] == [(2, 1, 1), (1, 1, 2), (2, 4, 1)]
    assert all(fused_form(K) == (2, 4) for K, _ in LONG_K)


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("name", list(SHAPES))
def test_layer_kernels_bitwise_equal_single_row_fp4(ops, name, B):
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
    # ---- yardstick: the single-row fp4 entries, lane by lane, on copies
    want = []
    for b, ln in enumerate(lanes):
        pool, lin = ln.pool.clone(), ln.lin.clone()
        q = torch.zeros(qd, dtype=BF16).cuda()
        ops.dec_qkv_fp4(x[b], w["ln"], 1e-6, *w["qkv"], w["qkv_b"], q, pool, layer, ln.slot_of, qd, kd, len_dev=ln.state[0:1], lin=(lin, ln.lin_len))
        xo = x[b].clone()
        ops.gemv_fp4(attn[b], *w["o"], residual=xo, out=xo)
        h = torch.zeros(I, dtype=BF16).cuda()
        ops.dec_gate_up_fp4(x[b], w["ln"], 1e-6, *w["gu"], h)
        xd = x[b].clone()
        ops.gemv_fp4(hrow[b], *w["down"], residual=xd, out=xd)
        want.append(dict(q=q, pool=pool, lin=lin, xo=xo, h=h, xd=xd))
    # ---- batched
    before = [ln.snapshot() for ln in lanes]
    q = torch.zeros((B, qd + 2 * kd), dtype=BF16).cuda()                  # (a group's q|k|v-wide buffer: the row stride is not qd)
    ops.decb_qkv_fp4(tab, B, x, w["ln"], 1e-6, *w["qkv"], w["qkv_b"], q, layer, qd, kd, D, N_LAYERS)
    xo = x.clone()
    ops.decb_gemv_fp4(tab, B, attn, *w["o"], xo, xo)
    h = torch.zeros((B, I), dtype=BF16).cuda()
    ops.decb_gate_up_fp4(tab, B, x, w["ln"], 1e-6, *w["gu"], h)
    xd = x.clone()
    ops.decb_gemv_fp4(tab, B, hrow, *w["down"], xd, xd)
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


# GEMV forms no model width reaches: (2, 1) with one K-step and N no multiple of the 8 rows of a workgroup; (1, 1) with two K-steps, the
# second holding one block; (2, 4) with odd N (a clamped second row) and 129 blocks split 33 / 33 / 33 / 30
EXTRA_GEMV = [(4098, 512), (250, 2080), (255, 4128)]


@pytest.mark.parametrize("B", [1, 2, 3, 4])
@pytest.mark.parametrize("N,K", EXTRA_GEMV)
def test_residual_gemv_other_forms_bitwise_equal_single_row_fp4(ops, N, K, B):
    W = q4((N, K), 13, 1.0 / np.sqrt(K))
    lanes = make_lanes(B, 2, 100)
    tab = lane_table(ops, lanes)
    x, res = rnd((B, K), 50 + B), rnd((B, N), 60 + B)
    y = res.clone()
    ops.decb_gemv_fp4(tab, B, x, *W, y, y)
    for b in range(B):
        want = res[b].clone()
        ops.gemv_fp4(x[b], *W, residual=want, out=want)
        same(f"y[{b}]", y[b], want)


# the fused kernels past K = 4096, <PRE, XC> = <2, 4>, where the K loop runs twice: the second batch holding one block; B * K * 2 =
# 65280, exactly the LDS cap; the longest row the entries take
LONG_K = [(4128, 2), (8160, 4), (8192, 3)]


@pytest.mark.parametrize("K,B", LONG_K)
def test_fused_kernels_on_rows_past_4096_bitwise_equal_single_row_fp4(ops, K, B):
    qd = kd = D                                    # one kv head
    I = 100                                        # no multiple of the 4 rows of a workgroup
    assert B * K * 2 <= 65536 - 256
    s = 1.0 / np.sqrt(K)
    ln_w, qkv, qkv_b, gu = rnd((K,), 1), q4((qd + 2 * kd, K), 2, s), rnd((qd + 2 * kd,), 3, 0.5), q4((2 * I, K), 5, s)
    lanes = make_lanes(B, 1, 100)
    tab = lane_table(ops, lanes)
    x = rnd((B, K), 70 + B)
    for b in range(B):
        x[b] *= (b + 1) * 0.7
    layer = 0
    want = []
    for b, ln in enumerate(lanes):
        pool, lin = ln.pool.clone(), ln.lin.clone()
        q = torch.zeros(qd, dtype=BF16).cuda()
        ops.dec_qkv_fp4(x[b], ln_w, 1e-6, *qkv, qkv_b, q, pool, layer, ln.slot_of, qd, kd, len_dev=ln.state[0:1], lin=(lin, ln.lin_len))
        h = torch.zeros(I, dtype=BF16).cuda()
        ops.dec_gate_up_fp4(x[b], ln_w, 1e-6, *gu, h)
        want.append(dict(q=q, pool=pool, lin=lin, h=h))
    q = torch.zeros((B, qd), dtype=BF16).cuda()
    ops.decb_qkv_fp4(tab, B, x, ln_w, 1e-6, *qkv, qkv_b, q, layer, qd, kd, D, N_LAYERS)
    h = torch.zeros((B, I), dtype=BF16).cuda()
    ops.decb_gate_up_fp4(tab, B, x, ln_w, 1e-6, *gu, h)
    torch.cuda.synchronize()
    for b, ln in enumerate(lanes):
        same(f"q[{b}]", q[b], want[b]["q"])
        same(f"pool[{b}]", ln.pool, want[b]["pool"])
        same(f"lin[{b}]", ln.lin, want[b]["lin"])
        same(f"h[{b}]", h[b], want[b]["h"])


@pytest.mark.parametrize("name", ["tiny", "2b"])
def test_inactive_lane_is_untouched_by_a_full_batched_fp4_step(ops, name):
    """A lane whose state says it is past its limit: every kernel of a step skips it -- pool, linear planes, tok_buf, state, seen and
    its rows of the group buffers keep their bits -- while the live lanes compute what they compute without it."""
    from test_decode_batch_fp8_gpu import q8
    H, I, hq, hkv = SHAPES[name]
    qd, kd = hq * D, hkv * D
    w = weights(name)
    V, B, dead = 3000, 3, 1
    table, head = rnd((V, H), 11), q8((V, H), 12, 1.0 / np.sqrt(H))          # (the lm_head of an fp4 engine is e4m3)
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
        ops.decb_qkv_fp4(tab, B, x, w["ln"], 1e-6, *w["qkv"], w["qkv_b"], q, 0, qd, kd, D, N_LAYERS)
        ops.decb_gemv_fp4(tab, B, q, *w["o"], x, x)
        ops.decb_gate_up_fp4(tab, B, x, w["ln"], 1e-6, *w["gu"], h)
        ops.decb_gemv_fp4(tab, B, h, *w["down"], x, x)
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
    lanes = make_lanes(4, 2, 100)
    tab = lane_table(ops, lanes)
    x = rnd((2, 256), 1)
    h5, h2 = torch.zeros((5, 512), dtype=BF16).cuda(), torch.zeros((2, 512), dtype=BF16).cuda()
    with pytest.raises(_lib.SvlmError):
        ops.decb_gate_up_fp4(tab, 5, x, w["ln"], 1e-6, *w["gu"], h5)                                  # B > 4 (wrapper)
    with pytest.raises(_lib.SvlmError):
        ops.decb_gate_up_fp4(tab, 2, x[:1], w["ln"], 1e-6, *w["gu"], h2)                              # too few x rows
    with pytest.raises(_lib.SvlmError):
        ops.decb_gemv_fp4(tab[:, :8].contiguous(), 2, x, *w["o"], x, x)                               # malformed lane table
    with pytest.raises(_lib.SvlmError):
        ops.decb_gemv_fp4(tab, 2, x, w["o"][0][:, :248], w["o"][1], x, x)                             # K = 496, no multiple of 32 (wrapper)
    with pytest.raises(_lib.SvlmError):
        ops.decb_gemv_fp4(tab, 2, x, w["o"][0], w["o"][1][:, :8].contiguous(), x, x)                  # too few block scales (wrapper)
    # the entry points' own checks, below the wrapper.  The buffers are large enough for every shape named, so a check that let one
    # through would still launch inside them
    gu4, gus = w["gu"]
    o4, os_ = w["o"]
    lib = ops.lib
    xl = torch.zeros((4, 8192), dtype=BF16).cuda()
    lnl = torch.ones(8192, dtype=BF16).cuda()
    w4l, sl = torch.zeros((1024, 4096), dtype=torch.uint8).cuda(), torch.full((1024, 256), 127, dtype=torch.uint8).cuda()
    out = torch.zeros((5, 512), dtype=BF16).cuda()

    def gate_up(B=2, K=256, ldw=4096, scale=sl):
        return lib.svlm_decb_gate_up_fp4(_ptr(tab), B, _ptr(xl), 8192, _ptr(lnl), 1e-6, _ptr(w4l), ldw, _ptr(scale), _ptr(out), 512, 512, K, _stream())

    def qkv(B=2, K=256, ldw=4096, scale=sl):
        return lib.svlm_decb_qkv_fp4(_ptr(tab), B, _ptr(xl), 8192, _ptr(lnl), 1e-6, _ptr(w4l), ldw, _ptr(scale), _ptr(lnl), _ptr(out), 512, 0, K,
                                     256, 256, D, _stream())

    def gemv(B=2, K=512, ldw=4096, scale=sl, residual=out):
        return lib.svlm_decb_gemv_fp4(_ptr(tab), B, _ptr(xl), 8192, _ptr(w4l), ldw, _ptr(scale), _ptr(residual), 512, _ptr(out), 512, 256, K, _stream())

    for what, rc in (("gate_up B=5", gate_up(B=5)), ("qkv B=5", qkv(B=5)), ("gemv B=5", gemv(B=5)),
                     ("gate_up K=8192 at B=4", gate_up(B=4, K=8192)), ("qkv K=8192 at B=4", qkv(B=4, K=8192)),
                     ("gate_up K=240", gate_up(K=240)), ("qkv K=240", qkv(K=240)), ("gemv K=496", gemv(K=496)),
                     ("gate_up null scales", gate_up(scale=None)), ("qkv null scales", qkv(scale=None)), ("gemv null scales", gemv(scale=None)),
                     ("gate_up ldw=4104", gate_up(ldw=4104)), ("qkv ldw=4104", qkv(ldw=4104)), ("gemv ldw=4104", gemv(ldw=4104)),
                     ("gemv ldw < K / 2", gemv(K=512, ldw=128)),
                     ("gemv null residual", gemv(residual=None))):
        assert rc != 0, f"{what}: accepted"
        with pytest.raises(_lib.SvlmError):
            ops._check(rc, what)
    # ... and the same helpers accept what they should (so the refusals above are not refusals of the helpers' other arguments)
    for what, rc in (("gate_up", gate_up()), ("qkv", qkv()), ("gemv", gemv()), ("gate_up K=8192 at B=3", gate_up(B=3, K=8192))):
        assert rc == 0, f"{what}: refused"
    torch.cuda.synchronize()
