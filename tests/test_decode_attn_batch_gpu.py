"""Lane-batched decode attention (svlm_decb_attn, csrc/decode_attn.hip: the attention of all lanes of a stream group's batch in one split
launch and one combine launch) through the C ABI.

The yardstick is BIT EQUALITY, per live lane, with `ops.decode_attn` called alone with that lane's arguments: the output row and the
whole workspace (partials included; NaN where the single-lane call leaves NaN).  The single-lane paths are held to the fp64 bound by
tests/test_attn_merge_gpu.py, whose inputs (`_case`: NaN in every pool slot the sequence does not map to, `iid` / `sink` generators,
`_lin_planes`: planes as the prefill leaves them) are used here; no second numeric bound and no tolerance.

A lane owns a two-layer pool (the attention runs on layer 1: the planes are addressed from the pool's base), its slot map, rope table,
state, workspace and possibly linear planes; lanes of a batch differ in length, n_slots, and -- in the ragged batches -- in attn_len,
chunk and kernel class.  The group buffers q / out are wider than Hq * D and out has a row more than the batch.
"""
import functools

import numpy as np
import pytest
import torch

from test_attn_merge_gpu import D, NAN, SCALE, _case, _lin_planes, decode_path
from test_decode_wide_gpu import bits, dead_set, same

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
LAYER = 1
SENTINEL = 0x7b7b
PAD = 256              # columns of the group buffers beyond Hq * D


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def refops():
    from ref_ops import RefOps
    return RefOps()


@functools.lru_cache(maxsize=None)
def _lane_case(refops, ident, Hq, Hkv, L, attn_len):
    """The lane's cache content, computed once per (ident, shape) and never modified: a lane keeps it whatever batch or column it is in."""
    return _case(refops, ("iid", "sink")[ident % 2], Hq, Hkv, L, 1, attn_len, 300 + 13 * ident + Hq, L // 2)


@functools.lru_cache(maxsize=None)
def _lane_planes(ops, refops, ident, Hq, Hkv, L, attn_len):
    return _lin_planes(ops, _lane_case(refops, ident, Hq, Hkv, L, attn_len), Hq, Hkv, L, attn_len)


class ALane:
    """One lane of a batch.  planes: None, "fresh" (lin_state = {L, 1} as the prefill leaves it) or "stale" ({L - 100, 0}: the rows
    above come from the pool).  dead: state[1] + 1 == limit.  nan_pool: nothing of the lane may be read (dead lanes only)."""

    def __init__(self, ops, refops, ident, Hq, Hkv, L, attn_len, chunk, planes=None, dead=False, nan_pool=False):
        c = _lane_case(refops, ident, Hq, Hkv, L, attn_len)
        self.ident, self.Hq, self.Hkv, self.L, self.attn_len, self.chunk, self.dead = ident, Hq, Hkv, L, attn_len, chunk, dead
        n0 = c["pool"].shape[3]
        self.n_slots = n0 + 16 * (ident % 3)
        self.pool = torch.full((2, 2, Hkv, self.n_slots, D), NAN, dtype=BF16, device="cuda")
        if not nan_pool:
            self.pool[LAYER, :, :, :n0] = c["pool"][0]
        self.slot_of, self.rope, self.q = c["slot_of"], c["rope"], c["q"][0]
        self.lin = self.lin_state = None
        if planes is not None:
            p1, _ = _lane_planes(ops, refops, ident, Hq, Hkv, L, attn_len)
            self.lin = torch.full((2,) + tuple(p1.shape[1:]), NAN, dtype=BF16, device="cuda")
            self.lin[LAYER] = p1[0]
            self.lin_state = torch.tensor([L, 1] if planes == "fresh" else [L - 100, 0], dtype=torch.int32, device="cuda")
        cur = 1
        self.state = torch.tensor([L - 1, cur], dtype=torch.int32, device="cuda")        # the length is state[0] + 1
        self.tok_buf = torch.zeros(12, dtype=torch.int32, device="cuda")
        self.limit = cur + 1 if dead else 11
        self.ws = ops.decode_attn_ws(Hq, attn_len, chunk, "cuda")

    def lin_arg(self):
        return None if self.lin is None else (self.lin, self.lin_state)

    def path(self):
        return decode_path(self.Hq, self.Hkv, self.L, self.attn_len, self.chunk, self.lin is not None)

    def alone(self, ops):
        """(out row, workspace) of the single-lane entry for this lane; the workspace is NaN before the call."""
        ws = torch.full_like(self.ws, NAN)
        out = torch.full((self.Hq * D,), NAN, dtype=BF16, device="cuda")
        ops.decode_attn(self.q, self.pool, LAYER, self.slot_of, self.rope, out, ws, self.Hq, self.attn_len, self.chunk, SCALE, length=1,
                        len_dev=self.state[0:1], lin=self.lin_arg())
        return out, ws


def tables(ops, lanes):
    lt = np.stack([ops.lane_record(ln.pool, ln.lin, ln.slot_of, ln.state, ln.tok_buf, None, ln.limit) for ln in lanes])
    at = np.stack([ops.lane_attn_record(ln.rope, ln.lin_state, ln.ws, ln.attn_len, ln.chunk, ln.Hq, slot_of=ln.slot_of, lin=ln.lin)
                   for ln in lanes])
    return torch.from_numpy(lt).cuda(), torch.from_numpy(at).cuda()


def batched(ops, lanes, columns=None, rows=None):
    """One svlm_decb_attn over `lanes` -> the group's out buffer.  Workspaces NaN, out sentinel-filled before the call."""
    B, Hq, Hkv = len(lanes), lanes[0].Hq, lanes[0].Hkv
    rows = rows or B + 1
    q = torch.full((rows, Hq * D + PAD), 0.5, dtype=BF16, device="cuda")
    for b, ln in enumerate(lanes):
        q[b, :Hq * D] = ln.q
        ln.ws.fill_(NAN)
    out = torch.full((rows, Hq * D + PAD), SENTINEL, dtype=torch.int16, device="cuda").view(BF16)
    lt, at = tables(ops, lanes)
    ops.decb_attn(lt, at, B, q, out, LAYER, Hq, SCALE, [ln.attn_len for ln in lanes], [ln.chunk for ln in lanes],
                  [ln.lin is not None for ln in lanes], Hkv)
    torch.cuda.synchronize()
    return out


def untouched(name, t):
    assert bool((bits(t) == SENTINEL).all()), f"{name}: written"


def check_batch(ops, lanes, name):
    """Every live lane: out row and workspace bitwise those of the lane alone.  Dead lanes, rows >= B, the columns beyond Hq * D, the
    pools and the planes: untouched."""
    B, Hq = len(lanes), lanes[0].Hq
    want = [None if ln.dead else ln.alone(ops) for ln in lanes]
    before = [(ln.pool.clone(), None if ln.lin is None else ln.lin.clone()) for ln in lanes]
    out = batched(ops, lanes)
    for b, ln in enumerate(lanes):
        if ln.dead:
            untouched(f"{name}: dead lane {b} out row", out[b])
            assert bool(torch.isnan(ln.ws).all()), f"{name}: dead lane {b}: workspace written"
            continue
        same(f"{name}: lane {b} {ln.path()} out", out[b, :Hq * D], want[b][0])
        same(f"{name}: lane {b} {ln.path()} workspace", ln.ws, want[b][1])
        assert not bool(torch.isnan(out[b, :Hq * D].float()).any()), f"{name}: lane {b}: NaN in the output"
        same(f"{name}: lane {b} pool", ln.pool, before[b][0])
        if ln.lin is not None:
            same(f"{name}: lane {b} planes", ln.lin, before[b][1])
    untouched(f"{name}: rows >= B", out[B:])
    untouched(f"{name}: columns beyond Hq * D", out[:, Hq * D:])
    return out


# ----------------------------------------------------------------------------- 1. path matrix
# name: (Hq, Hkv, attn_len, chunk, planes, Ls of the three lanes)
_PATHS = {
    "split16": (12, 2, 1024, 16, None, (1000, 700, 333)),
    "split48": (12, 2, 1024, 48, None, (1000, 700, 333)),
    "split64": (12, 2, 1024, 64, None, (1000, 700, 333)),
    "split48-planes": (12, 2, 1024, 48, "fresh", (1000, 700, 333)),
    "streampool128": (12, 2, 1024, 128, None, (1000, 700, 333)),
    "streamlin128": (12, 2, 1024, 128, "fresh", (1000, 700, 333)),
    "streamlin128-stale": (12, 2, 1024, 128, "stale", (1000, 700, 333)),
    "combine-DS1": (12, 2, 1024, 48, None, (1001, 650, 48)),
    "combine-DS2": (12, 2, 2176, 16, None, (2052, 1100, 17)),
    "combine-DS4": (12, 2, 3200, 16, None, (3100, 1900, 100)),
}
for _form, (_chunk, _planes) in enumerate([(48, None), (128, None), (128, "fresh")]):
    for _G in range(1, 9):
        _hkv = 1 + (_G + _form) % 2
        _PATHS[f"G{_G}-c{_chunk}-{_planes or 'pool'}"] = (_G * _hkv, _hkv, 1024, _chunk, _planes, (1000, 990, 520))


def test_the_matrix_reaches_every_kernel_and_combine_form():
    reached = set()
    for Hq, Hkv, attn_len, chunk, planes, Ls in _PATHS.values():
        kernel, ds = decode_path(Hq, Hkv, Ls[0], attn_len, chunk, planes is not None)[:2]
        reached.add((kernel, ds, Hq // Hkv))
    assert {(k, ds) for k, ds, _ in reached} >= {("split", 1), ("split", 2), ("split", 4), ("streampool", 1), ("streamlin", 1)}
    for kernel in ("split", "streampool", "streamlin"):
        assert {g for k, _, g in reached if k == kernel} >= set(range(1, 9)), kernel


@pytest.mark.parametrize("name", list(_PATHS))
def test_every_path_is_bitwise_the_single_lane_call(ops, refops, name):
    Hq, Hkv, attn_len, chunk, planes, Ls = _PATHS[name]
    lanes = [ALane(ops, refops, 10 + i, Hq, Hkv, L, attn_len, chunk, planes) for i, L in enumerate(Ls)]
    assert len({ln.n_slots for ln in lanes}) == 3
    check_batch(ops, lanes, name)


# ----------------------------------------------------------------------------- 2. ragged batches
def test_lanes_of_one_class_differ_in_attn_len_and_chunk(ops, refops):
    geo = [(1024, 16, 1000), (2048, 48, 1500), (3072, 48, 3000)]
    lanes = [ALane(ops, refops, 20 + i, 12, 2, L, a, c) for i, (a, c, L) in enumerate(geo)]
    assert {ln.path()[:2] for ln in lanes} == {("split", 1)} and len({ln.path()[4] for ln in lanes}) == 2
    check_batch(ops, lanes, "ragged one class")


def test_a_batch_of_mixed_classes(ops, refops):
    geo = [(1024, 48, 1000, None), (1024, 128, 900, "fresh"), (1024, 128, 800, None), (2176, 16, 2052, None), (3200, 16, 3100, None),
           (1024, 128, 1000, "stale"), (1024, 64, 64, "fresh")]
    lanes = [ALane(ops, refops, 30 + i, 12, 2, L, a, c, p) for i, (a, c, L, p) in enumerate(geo)]
    assert {ln.path()[0] for ln in lanes} == {"split", "streamlin", "streampool"} and {ln.path()[1] for ln in lanes} == {1, 2, 4}
    check_batch(ops, lanes, "mixed classes")


@pytest.mark.parametrize("B", [1, 16])
def test_one_lane_and_sixteen(ops, refops, B):
    lanes = [ALane(ops, refops, 40 + i, 12, 2, 1000 - 61 * i, 1024, 48, "fresh" if i % 3 == 0 else None) for i in range(B)]
    check_batch(ops, lanes, f"B={B}")


# ----------------------------------------------------------------------------- 3. side effects
@pytest.mark.parametrize("B,chunk", [(4, 48), (16, 128)])
def test_dead_lanes_and_everything_else_stay_untouched(ops, refops, B, chunk):
    lanes = [ALane(ops, refops, 50 + i, 12, 2, 1000 - 37 * i, 1024, chunk, "fresh" if i % 2 else None, dead=i in dead_set(B))
             for i in range(B)]
    assert sum(ln.dead for ln in lanes) == 2
    check_batch(ops, lanes, f"dead lanes B={B} chunk={chunk}")


# ----------------------------------------------------------------------------- 4. lane placement
@pytest.mark.parametrize("chunk,planes", [(48, None), (128, "fresh")])
def test_a_lane_does_not_depend_on_its_place_or_its_neighbours(ops, refops, chunk, planes):
    Hq, Hkv = 12, 2

    def me():
        return ALane(ops, refops, 60, Hq, Hkv, 1000, 1024, chunk, planes)

    def other(i, **kw):
        return ALane(ops, refops, 61 + i, Hq, Hkv, 900 - 50 * i, 1024, chunk, planes, **kw)

    alone = batched(ops, [me()])[0, :Hq * D].clone()
    first = batched(ops, [me()] + [other(i) for i in range(15)])[0, :Hq * D].clone()
    last = batched(ops, [other(i) for i in range(15)] + [me()])[15, :Hq * D].clone()
    beside_dead = batched(ops, [other(0, dead=True, nan_pool=True), me()])[1, :Hq * D].clone()
    for name, got in (("column 0 of 16", first), ("column 15 of 16", last), ("beside a dead lane full of NaN", beside_dead)):
        same(name, got, alone)
    same("the single-lane call", alone, me().alone(ops)[0])


# ----------------------------------------------------------------------------- 5. determinism and refusals
def test_two_calls_give_equal_bits(ops, refops):
    lanes = [ALane(ops, refops, 70 + i, 12, 2, 1000 - 100 * i, 1024, c, p) for i, (c, p) in enumerate([(48, None), (128, "fresh"), (128, None)])]
    a = batched(ops, lanes)
    wa = [ln.ws.clone() for ln in lanes]
    b = batched(ops, lanes)
    same("out", a, b)
    for ln, w in zip(lanes, wa):
        same("workspace", ln.ws, w)


def test_refusals_write_nothing(ops, refops):
    from streaming_vlm_amd._lib import SvlmError
    Hq, Hkv = 12, 2
    lanes = [ALane(ops, refops, 80 + i, Hq, Hkv, 500, 1024, 48) for i in range(2)]
    lt, at = tables(ops, lanes)
    big_lt = torch.zeros((17, ops.LANE_WORDS), dtype=torch.int64, device="cuda")
    big_at = torch.zeros((17, ops.ATTN_WORDS), dtype=torch.int64, device="cuda")
    q = torch.full((17, Hq * D + PAD), 0.5, dtype=BF16, device="cuda")
    out = torch.full((17, Hq * D + PAD), SENTINEL, dtype=torch.int16, device="cuda").view(BF16)
    for ln in lanes:
        ln.ws.fill_(NAN)

    def call(lt_, at_, B, Hq_=Hq, Hkv_=Hkv, chunks=None):
        ops.decb_attn(lt_, at_, B, q, out, LAYER, Hq_, SCALE, [1024] * B, chunks or [48] * B, [False] * B, Hkv_)

    with pytest.raises(SvlmError):
        call(lt, at, 0)
    with pytest.raises(SvlmError):
        call(big_lt, big_at, 17)
    with pytest.raises(SvlmError):
        call(lt, None, 2)
    with pytest.raises(SvlmError):
        call(None, at, 2)
    with pytest.raises(SvlmError):
        call(lt, at, 2, chunks=[48, 24])                        # an illegal chunk in one lane
    with pytest.raises(SvlmError):
        call(lt, at, 2, chunks=[48, 576])
    with pytest.raises(SvlmError):
        ops.lane_attn_record(lanes[1].rope, None, lanes[1].ws, 1024, 24, Hq)      # ... and in its record
    with pytest.raises(SvlmError):
        call(lt, at, 2, Hq_=9, Hkv_=1)                          # a head group of 9
    with pytest.raises(SvlmError):
        call(lt, at, 2, Hq_=12, Hkv_=5)
    # the library's own checks, behind the wrapper's: same refusals from the C entry, no launch
    import ctypes
    host = (ctypes.c_int * 6)(1024, 1024, 48, 48, 0, 0)
    h = ctypes.addressof(host)
    bad = (ctypes.c_int * 6)(1024, 1024, 48, 24, 0, 0)
    hb = ctypes.addressof(bad)
    lib, P = ops.lib, lambda t: t.data_ptr()

    def c_call(lt_=P(lt), at_=P(at), B=2, Hq_=Hq, Hkv_=Hkv, D_=D, hh=h):
        return lib.svlm_decb_attn(lt_, at_, B, P(q), q.stride(0), P(out), out.stride(0), LAYER, Hq_, Hkv_, D_, SCALE, hh, hh + 8, hh + 16, None)

    assert lib.svlm_decb_attn_max_lanes() == 16 == ops.decb_attn_max_lanes()
    for kw in (dict(B=0), dict(B=17), dict(lt_=None), dict(at_=None), dict(hh=hb), dict(Hq_=9, Hkv_=1), dict(D_=64)):
        assert c_call(**kw) != 0, kw
    torch.cuda.synchronize()
    untouched("out after the refusals", out)
    for ln in lanes:
        assert bool(torch.isnan(ln.ws).all())
    call(lt, at, 2)                                                 # (the same arguments, legal: it runs)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out[:2, :Hq * D].float()).any()) and not bool((bits(out[:2, :Hq * D]) == SENTINEL).all())
