"""Where the seven qkv kernels put the new token's K / V row, against the Python reference.

All of them place it through one device function (csrc/dec_epi.h: kv_append), and the lane-batched suites compare the lane-batched
kernels with the single-row kernel of their format -- the same function on both sides.  Here every entry is held to RefOps.dec_qkv
(tests/ref_ops.py) on the CPU instead, with the format's dequantised weights as ref_ops_fp8 / ref_ops_fp4 do it:

  (a) the set of pool and linear-plane elements that changed is exactly the set the reference changes (the other layer, the other
      slots and the other rows keep their sentinel bits);
  (b) the key row read back with RefOps.lin_k_rows and the value row of the planes are bitwise the pool's slot row;
  (c) the written values agree with the reference to the tolerance of the qkv-against-reference tests of the format
      (test_kernels_gpu.py / test_llm_fp8_gpu.py / test_llm_fp4_gpu.py: `close`, max 2^-7 and mean 1e-3 of the largest value);
  (d) a lane that is not live changes nothing in its pool, planes or q row.

Shapes: Hq = Hkv = 2, D = 128 (qd = kd = 256), K = 256, two layers of which layer 1 is written, permuted slot tables; lanes differ in
logical row (tile 1 row 5, tile 2 row 5, tile 0 row 5, tile 1 row 14), n_slots (24 / 40) and lin_rows (32 / 48).
"""
import functools

import numpy as np
import pytest
import torch

from ref_ops import RefOps
from test_kernels_gpu import close

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D, HQ, HKV, K = 128, 2, 2, 256
QD, KD = HQ * D, HKV * D
N_LAYERS, LAYER = 2, 1
EPS = 1e-6
SENTINEL = 0x7b7b              # a finite bf16 bit pattern (1.3e36) no output here takes
# a lane's own geometry: (logical row, n_slots, lin_rows); its x row and slot table are seeded by its index here
SPECS = [(21, 24, 32), (37, 40, 48), (5, 24, 32), (30, 40, 48)]
DEAD = (21, 24, 32)
FORMATS = ["bf16", "fp8", "fp4"]


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


def rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def sentinel(shape, device="cpu"):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=device).view(BF16)


def touched(t):
    return t.view(torch.int16).cpu() != SENTINEL


def same_bits(a, b):
    return torch.equal(a.cpu().view(torch.int16), b.cpu().view(torch.int16))


LNW = rnd((K,), 2, 0.1) + 1
BIAS = rnd((QD + 2 * KD,), 4, 0.1)


@functools.lru_cache(maxsize=None)
def weights(fmt):
    """(the entry's weight arguments on the GPU, W' on the host)."""
    N = QD + 2 * KD
    if fmt == "bf16":
        W = rnd((N, K), 3, 0.03)
        return (W.cuda(),), W
    if fmt == "fp8":
        from streaming_vlm_amd.weights import dequantize_rows_fp8, quantize_rows_fp8_pow2
        mag = 10.0 ** (torch.rand((N, 1), generator=torch.Generator().manual_seed(1003)) * 2 - 1)
        q, s = quantize_rows_fp8_pow2((rnd((N, K), 3, 0.03).float() * mag).to(BF16))
        return (q.cuda(), s.cuda()), dequantize_rows_fp8(q, s)
    from streaming_vlm_amd.weights import dequantize_blocks_mxfp4, quantize_blocks_mxfp4
    g = torch.Generator().manual_seed(2003)
    mag = 10.0 ** (torch.rand((N, 1, 1), generator=g) * 2 - 1 + torch.rand((N, K // 32, 1), generator=g) * 2 - 1)
    w = (rnd((N, K), 3, 0.03).float().view(N, K // 32, 32) * mag).view(N, K).to(BF16)
    codes, scales = quantize_blocks_mxfp4(w.cuda())
    return (codes, scales), dequantize_blocks_mxfp4(codes, scales).cpu()


def x_row(i):
    return rnd((K,), 100 + i, 2.0)


def slot_table(i, n_slots):
    return torch.randperm(n_slots, generator=torch.Generator().manual_seed(60 + i)).to(torch.int32)


@functools.lru_cache(maxsize=None)
def reference(fmt, i):
    """RefOps.dec_qkv for lane spec i on sentinel-filled storage: (q, pool, planes), computed once and left unchanged."""
    row, n_slots, lin_rows = SPECS[i]
    q, pool, planes = sentinel((QD,)), sentinel((N_LAYERS, 2, HKV, n_slots, D)), sentinel((N_LAYERS, 2, HKV, lin_rows, D))
    RefOps().dec_qkv(x_row(i), LNW, EPS, weights(fmt)[1], BIAS, q, pool, LAYER, slot_table(i, n_slots), QD, KD, length=row, lin=(planes, None))
    # the reference itself writes one slot row and one logical row of layer 1, both planes, every kv head
    assert int(touched(pool).sum()) == int(touched(pool[LAYER, :, :, int(slot_table(i, n_slots)[row])]).sum()) == 2 * HKV * D
    assert int(touched(planes).sum()) == int(touched(planes[LAYER]).sum()) == 2 * HKV * D
    return q, pool, planes


def check_written(name, fmt, i, q, pool, planes):
    row, n_slots, _ = SPECS[i]
    q_ref, pool_ref, planes_ref = reference(fmt, i)
    slot = int(slot_table(i, n_slots)[row])
    # (a)
    assert torch.equal(touched(pool), touched(pool_ref)), f"{name}: the pool elements written are not the reference's"
    assert torch.equal(touched(planes), touched(planes_ref)), f"{name}: the linear-plane elements written are not the reference's"
    assert bool(touched(q).all()), f"{name}: q columns left unwritten"
    # (b)
    pool, planes = pool.cpu(), planes.cpu()
    k_row, v_row = pool[LAYER, 0][:, slot], pool[LAYER, 1][:, slot]
    assert same_bits(RefOps.lin_k_rows(planes[LAYER, 0], row + 1)[:, row], k_row), f"{name}: key row of the planes is not the pool's"
    assert same_bits(planes[LAYER, 1][:, row], v_row), f"{name}: value row of the planes is not the pool's"
    # (c)
    close(f"{name} q", q, q_ref)
    close(f"{name} k", k_row, pool_ref[LAYER, 0][:, slot])
    close(f"{name} v", v_row, pool_ref[LAYER, 1][:, slot])


@pytest.mark.parametrize("fmt", FORMATS)
def test_single_row_qkv_places_the_row_where_the_reference_does(ops, fmt):
    entry = {"bf16": ops.dec_qkv, "fp8": ops.dec_qkv_fp8, "fp4": ops.dec_qkv_fp4}[fmt]
    row, n_slots, lin_rows = SPECS[0]
    for how in ("host", "device"):               # both length forms
        q, pool = sentinel((QD,), "cuda"), sentinel((N_LAYERS, 2, HKV, n_slots, D), "cuda")
        planes, lin_state = sentinel((N_LAYERS, 2, HKV, lin_rows, D), "cuda"), torch.tensor([row, 1], dtype=torch.int32, device="cuda")
        length = dict(length=row) if how == "host" else dict(len_dev=torch.tensor([row], dtype=torch.int32, device="cuda"))
        entry(x_row(0).cuda(), LNW.cuda(), EPS, *weights(fmt)[0], BIAS.cuda(), q, pool, LAYER, slot_table(0, n_slots).cuda(), QD, KD,
              lin=(planes, lin_state), **length)
        check_written(f"dec_qkv[{fmt}, {how} length]", fmt, 0, q, pool, planes)


class Lane:
    """What one lane owns, on the GPU, sentinel-filled; spec None: a lane that is not live (state[1] + 1 == limit)."""

    def __init__(self, i):
        self.i = i
        row, n_slots, lin_rows = DEAD if i is None else SPECS[i]
        self.pool, self.lin = sentinel((N_LAYERS, 2, HKV, n_slots, D), "cuda"), sentinel((N_LAYERS, 2, HKV, lin_rows, D), "cuda")
        self.slot_of = slot_table(9 if i is None else i, n_slots).cuda()
        self.state = torch.tensor([row, 3], dtype=torch.int32).cuda()
        self.tok_buf = torch.zeros(12, dtype=torch.int32).cuda()
        self.limit = 4 if i is None else 10
        self.x = x_row(9 if i is None else i)

    def record(self, ops):
        return ops.lane_record(self.pool, self.lin, self.slot_of, self.state, self.tok_buf, None, self.limit)


def run_lanes(ops, entry, fmt, name, order):
    lanes = [Lane(i) for i in order]
    B = len(lanes)
    tab = torch.from_numpy(np.stack([ln.record(ops) for ln in lanes])).cuda()
    x = torch.stack([ln.x for ln in lanes]).cuda()
    q = sentinel((B, QD), "cuda")
    entry(tab, B, x, LNW.cuda(), EPS, *weights(fmt)[0], BIAS.cuda(), q, LAYER, QD, KD, D, N_LAYERS)
    torch.cuda.synchronize()
    for b, ln in enumerate(lanes):
        if ln.i is None:                         # (d)
            assert not bool(touched(ln.pool).any()) and not bool(touched(ln.lin).any()) and not bool(touched(q[b]).any()), \
                f"{name}: lane {b} is not live and was written"
        else:
            check_written(f"{name} lane {b}", fmt, ln.i, q[b], ln.pool, ln.lin)
        assert ln.state.tolist() == [(DEAD if ln.i is None else SPECS[ln.i])[0], 3], f"{name}: lane {b} state changed"


@pytest.mark.parametrize("fmt", FORMATS)
def test_lane_batched_qkv_places_each_live_lanes_row_where_the_reference_does(ops, fmt):
    entry = {"bf16": ops.decb_qkv, "fp8": ops.decb_qkv_fp8, "fp4": ops.decb_qkv_fp4}[fmt]
    run_lanes(ops, entry, fmt, f"decb_qkv[{fmt}]", [0, None, 1])


def test_wide_qkv_places_each_live_lanes_row_where_the_reference_does(ops):
    run_lanes(ops, ops.decw_qkv, "bf16", "decw_qkv", [0, 1, 2, None, 3])
