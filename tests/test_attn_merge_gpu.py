"""Every split / merge path of the decode and prefill attention against the fp64 reference (tests/attn_ref64.py).

Decode and prefill attention cut the key range into splits whose (m, l, O) partials a merge kernel rescales by exp(m_s - M) and sums:
decode_attn_split_kernel (chunk <= 64) or decode_attn_stream_kernel (pool or linear planes, chunk 128..512), then
decode_attn_combine_kernel<NW, DS> with DS = 1, 2, 4; the prefill's up to 8 key splits merged by flash_combine_kernel.  Each case id
names the path a small Python mirror of the dispatch rules says it reaches (kernel, DS, combine batches, live / allocated splits).

Score generators (identity rope table in all but `iid`, so key content sets the scores directly):
  iid         randn q, K, V under an M-RoPE table (no split dominates)
  sink        keys 0..3 about ln((L-4)/4) nats above the rest: sinks and body carry about half the weight each (a wrong rescale of
              the first split against the others moves the output by a quarter of E)
  sink30      keys 0..3 30 nats above the rest (sink-dominated)
  late_spike  one key of the LAST live split 40 nats above everything: the running maximum moves in the last batch of the merge
  all_low     every score about -200 nats (only relative values matter; the -1e30 sentinels and > -1e29 guards must not bite)
  uniform     q = 0: the exact mean of V over the whole cache
Bound: |out - ref64| <= 2^-8 E + 2^-8 |ref64| per element and a mean bound (tests/attn_ref64.py).  The decode workspace is NaN before
every call (stale partial slots must be skipped), rows of the pool the sequence does not map to and linear-plane rows above the
prefill's are NaN as well.  Measured on MI355X: worst 0.78 of the per-element bound (sink30, 256 splits; sink-dominated cases sit
highest because the bf16 rounding of the few P entries that carry the weight does not average out), mean at most 0.69 x 2^-10; the
whole file runs in ~10 s.
"""
import functools
import math

import pytest
import torch

from attn_ref64 import attend64, check

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 128
SCALE = 1 / math.sqrt(D)
NAN = float("nan")
FIVE = ("iid", "sink", "late_spike", "all_low", "uniform")


# ----------------------------------------------------------------------------- Python mirrors of the dispatch rules
DA_CB = 12        # combine batch (decode_attn.hip)
FA_KT = 32        # prefill key tile (flash_attn.hip)


def decode_path(Hq, Hkv, L, max_len, chunk, lin):
    """svlm_decode_attn_lin: split kernel up to 64 keys per workgroup, else the streaming kernel (from the linear planes when given);
    combine DS = 4 above 192 allocated splits (16 waves), 2 above 64 (4 waves), else 1; NW * DS * DA_CB live splits per batch."""
    kernel = "split" if chunk <= 64 else ("streamlin" if lin else "streampool")
    ns_max = -(-max_len // chunk)
    ds = 4 if ns_max > 192 else (2 if ns_max > 64 else 1)
    nw = 16 if ds == 4 else 4
    ns = -(-L // chunk)
    return kernel, ds, -(-ns // (nw * ds * DA_CB)), ns, ns_max


def prefill_splits(T, L, Hq):
    """flash_attn.hip prefill_splits: ~480 workgroups, at least four 32-key tiles per split, 1..8."""
    base = -(-T // 64) * Hq
    ns = (480 + base // 2) // base if base > 0 else 1
    ns = min(ns, L // (4 * FA_KT))
    return max(1, min(8, ns))


def prefill_last_split(L, ns):
    """(index, first key) of the last non-empty key split of the LAST query tile (it sees every key): `per` tiles per split, even."""
    n_kt = -(-L // FA_KT)
    per = ((n_kt + ns - 1) // ns + 1) & ~1
    sp = (n_kt - 1) // per
    return sp, sp * per * FA_KT


# ----------------------------------------------------------------------------- inputs
@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def refops():
    from ref_ops import RefOps
    return RefOps()


def _a(nats):
    """per-dimension key value that scores `nats` against a query of ones"""
    return nats / (D * SCALE)


@functools.lru_cache(maxsize=2)
def _base(Hkv, L, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((Hkv, L, D), generator=g), torch.randn((Hkv, L, D), generator=g)


def _inputs(gen, Hq, Hkv, L, T, seed, spike):
    """-> q (T, Hq, D), K (Hkv, L, D), V (Hkv, L, D) float32 before the bf16 cast; identity rope for every generator but iid."""
    K0, V = _base(Hkv, L, seed)
    g = torch.Generator().manual_seed(seed + 7)
    if gen in ("iid", "uniform"):
        q = torch.randn((T, Hq, D), generator=g)
        K = K0
        if gen == "uniform":
            q = torch.zeros_like(q)
        return q, K, V
    q = 1.0 + 0.05 * torch.randn((T, Hq, D), generator=g)
    K = 0.25 * K0                                            # body scores ~ N(0, 1/16)
    if gen == "sink":
        K[:, :4] += _a(math.log(max(L - 4, 1) / 4))
    elif gen == "sink30":
        K[:, :4] += _a(30.0)
    elif gen == "late_spike":
        K[:, spike] += _a(40.0)
    elif gen == "all_low":
        K = K + _a(-200.0)
    else:
        raise ValueError(gen)
    return q, K, V


def _rope(refops, gen, cap, seed):
    if gen == "iid":
        pos3 = torch.randint(0, 3000, (3, cap), generator=torch.Generator().manual_seed(seed + 2), dtype=torch.int32)
        inv = 1.0 / (1e6 ** (torch.arange(0, D, 2, dtype=torch.float) / D))
        rope = torch.zeros((cap, D), dtype=BF16)
        refops.mrope_table(pos3, inv, rope, 0, cap, [16, 24, 24])
        return rope
    rope = torch.zeros((cap, D), dtype=BF16)
    rope[:, :D // 2] = 1.0                                   # cos = 1, sin = 0: the rotation is the identity, bit for bit
    return rope


def _case(refops, gen, Hq, Hkv, L, T, cap, seed, spike):
    """Pool (NaN in every slot the sequence does not map to), slot table, rope table, q rows and the fp64 reference of its last T
    query positions (causal)."""
    q, K, V = _inputs(gen, Hq, Hkv, L, T, seed, spike)
    q, K, V = q.to(BF16), K.to(BF16), V.to(BF16)
    n_slots = cap + 32
    slot_of = torch.randperm(n_slots, generator=torch.Generator().manual_seed(seed + 1)).to(torch.int32)[:cap].contiguous()
    pool = torch.full((1, 2, Hkv, n_slots, D), NAN, dtype=BF16)
    sl = slot_of[:L].long()
    pool[0, 0][:, sl] = K
    pool[0, 1][:, sl] = V
    rope = _rope(refops, gen, cap, seed)
    q_rot = refops._rot(q.transpose(0, 1), rope, torch.arange(L - T, L))          # (Hq, T, D) bf16, the kernels' bits
    K_rot = refops._rot(K, rope, torch.arange(L))
    ref, E = attend64(q_rot, K_rot, V, L - T, SCALE)
    return {"pool": pool.cuda(), "slot_of": slot_of.cuda(), "rope": rope.cuda(), "q": q.reshape(T, Hq * D).contiguous().cuda(),
            "ref": ref, "E": E}


def _lin_planes(ops, c, Hq, Hkv, L, cap):
    """Linear planes as the prefill leaves them (svlm_prefill_attn_ropeload_lin over the whole cache: rows [0, L) rotated,
    lin_state = {L, 1}); rows above L stay NaN."""
    lin_rows = -(-cap // 16) * 16
    planes = torch.full((1, 2, Hkv, lin_rows, D), NAN, dtype=BF16, device="cuda")
    lin_state = torch.zeros(2, dtype=torch.int32, device="cuda")
    T = min(16, L)
    qp = torch.randn((T, Hq * D), generator=torch.Generator().manual_seed(5)).to(BF16).cuda()
    out_p = torch.empty((T, Hq * D), dtype=BF16, device="cuda")
    ops.prefill_attn(qp, c["pool"], 0, c["slot_of"], c["rope"], out_p, T, L, Hq, SCALE, lin=(planes, lin_state))
    assert lin_state.tolist() == [L, 1]
    return planes, lin_state


# ----------------------------------------------------------------------------- decode
# (Hq, Hkv, L, max_len, chunk, lin, generators)
_DECODE_ROWS = [
    (12, 2, 3000, 3072, 48, False, FIVE),             # split, DS=1, 63 of 64 splits: 2 batches
    (12, 2, 2052, 2176, 16, False, ("iid", "sink")),  # split, DS=2, 129 of 136 splits: 2 batches
    (12, 2, 3100, 3200, 16, False, FIVE),             # split, DS=4, 194 of 200 splits
    (4, 2, 13000, 13056, 16, False, FIVE),            # split, DS=4, 813 of 816 splits: 2 batches
    (12, 2, 100, 4096, 16, False, FIVE),              # split, DS=4, 7 of 256 splits live: stale (NaN) slots skipped
    (12, 2, 32768, 32768, 128, False, FIVE),          # streaming from the pool, DS=4, 256 splits
    (12, 2, 131072, 131072, 512, True, FIVE),         # streaming from the linear planes, DS=4: bench.py's roofline_decode_attn_long (2B)
    (28, 4, 32768, 32768, 192, True, ("iid", "sink")),  # streaming from the linear planes, DS=2, 171 splits (7B heads at 32k keys)
    (12, 2, 3000, 3072, 48, False, ("sink30",)),
    (12, 2, 32768, 32768, 128, False, ("sink30",)),
]
# every head-group template G = 1..8 of the three split-kernel forms (split 48, streaming pool 128, streaming linear planes 128)
for _form, (_chunk, _lin) in enumerate([(48, False), (128, False), (128, True)]):
    for _G in range(1, 9):
        _hkv = 1 + (_G + _form) % 2
        _DECODE_ROWS.append((_G * _hkv, _hkv, 1000, 1024, _chunk, _lin, ("iid", "sink")))


def _decode_params():
    out = []
    for Hq, Hkv, L, max_len, chunk, lin, gens in _DECODE_ROWS:
        kernel, ds, nb, ns, ns_max = decode_path(Hq, Hkv, L, max_len, chunk, lin)
        for gen in gens:
            out.append(pytest.param(Hq, Hkv, L, max_len, chunk, lin, gen,
                                    id=f"{kernel}-DS{ds}-b{nb}-ns{ns}of{ns_max}-G{Hq // Hkv}-Hq{Hq}Hkv{Hkv}-L{L}-c{chunk}-{gen}"))
    return out


@functools.lru_cache(maxsize=1)
def _decode_case(refops, gen, Hq, Hkv, L, max_len):
    last16 = (-(-L // 16) - 1) * 16          # the spike: middle of the last 16-key tile, which lies in the last live split of every chunk
    spike = last16 + (L - last16) // 2
    c = _case(refops, gen, Hq, Hkv, L, 1, max_len, 100 + Hq + L, spike)
    c["spike"] = spike
    return c


@pytest.mark.parametrize("Hq,Hkv,L,max_len,chunk,lin,gen", _decode_params())
def test_decode_split_merge_vs_fp64(ops, refops, Hq, Hkv, L, max_len, chunk, lin, gen):
    kernel, ds, nb, ns, ns_max = decode_path(Hq, Hkv, L, max_len, chunk, lin)
    c = _decode_case(refops, gen, Hq, Hkv, L, max_len)
    if gen == "late_spike":
        assert (ns - 1) * chunk <= c["spike"] < L, "the spike must sit in the last live split"
    pg, sg, rg, q = c["pool"], c["slot_of"], c["rope"], c["q"][0]
    ws = ops.decode_attn_ws(Hq, max_len, chunk, "cuda")
    name = f"decode {kernel} DS{ds} batches{nb} splits {ns}/{ns_max} G{Hq // Hkv} Hkv{Hkv} L{L} chunk{chunk} {gen}"

    def run(lin_arg=None, dev_len=False):
        ws.fill_(NAN)                                        # stale partial slots must never be read
        out = torch.full((Hq * D,), NAN, dtype=BF16, device="cuda")
        if dev_len:
            len_dev = torch.tensor([L - 1], dtype=torch.int32, device="cuda")
            ops.decode_attn(q, pg, 0, sg, rg, out, ws, Hq, max_len, chunk, SCALE, length=1, len_dev=len_dev, lin=lin_arg)
        else:
            ops.decode_attn(q, pg, 0, sg, rg, out, ws, Hq, max_len, chunk, SCALE, length=L, lin=lin_arg)
        return out

    out = run()
    check(name, out.view(Hq, 1, D), c["ref"], c["E"])
    assert torch.equal(run(dev_len=True), out), f"{name}: device-length call differs"
    if lin:
        planes = _lin_planes(ops, c, Hq, Hkv, L, max_len)
        got = run(planes)
        assert torch.equal(got, out), f"{name}: linear planes and pool path differ"
        assert torch.equal(run(planes, dev_len=True), out), f"{name}: linear planes, device-length call differs"


# ----------------------------------------------------------------------------- prefill key splits
# (Hq, Hkv, T, L): the steady 2B chunk (8 splits), the 7B chunk (3), a T >= 1024 one-split case (two query blocks per wave), 5 and 2
_PREFILL_ROWS = [(12, 2, 275, 2330), (28, 4, 300, 4400), (28, 4, 1024, 1024), (12, 2, 480, 1500), (12, 2, 100, 300)]


def _prefill_params():
    out = []
    for Hq, Hkv, T, L in _PREFILL_ROWS:
        ns = prefill_splits(T, L, Hq)
        qb = 2 if (T >= 1024 and ns == 1) else 1
        for gen in ("iid", "sink", "late_spike"):
            out.append(pytest.param(Hq, Hkv, T, L, gen, id=f"splits{ns}-qb{qb}-Hq{Hq}Hkv{Hkv}-T{T}-L{L}-{gen}"))
    return out


def test_prefill_split_counts_of_the_sweep():
    """the sweep reaches 1, 2, 3, 5 and 8 key splits (mirror of prefill_splits)"""
    assert sorted(prefill_splits(T, L, Hq) for Hq, Hkv, T, L in _PREFILL_ROWS) == [1, 2, 3, 5, 8]


@pytest.mark.parametrize("Hq,Hkv,T,L,gen", _prefill_params())
def test_prefill_key_split_merge_vs_fp64(ops, refops, Hq, Hkv, T, L, gen):
    ns = prefill_splits(T, L, Hq)
    sp, lo = prefill_last_split(L, ns)
    spike = max(lo, L - 1 - T // 4)
    # the spike lies in the last key split and only the chunk's late rows see it (row i sees keys <= L - T + i)
    assert lo <= spike < L and spike > L - T
    cap = -(-L // 64) * 64
    c = _case(refops, gen, Hq, Hkv, L, T, cap, 200 + Hq + L, spike)
    pg, sg, rg, q = c["pool"], c["slot_of"], c["rope"], c["q"]
    name = f"prefill splits{ns} (spike in split {sp}) Hq{Hq} Hkv{Hkv} T{T} L{L} {gen}"

    def run(lin_arg=None):
        ws = ops._gemm_ws.get("pf" + str(q.device))           # the prefill's cached workspace (rotated rows, split partials): poisoned
        if ws is not None:
            ws.fill_(NAN)
        out = torch.full((T, Hq * D), NAN, dtype=BF16, device="cuda")
        ops.prefill_attn(q, pg, 0, sg, rg, out, T, L, Hq, SCALE, lin=lin_arg)
        return out

    out = run()
    check(name, out.view(T, Hq, D).transpose(0, 1), c["ref"], c["E"])
    lin_rows = -(-cap // 16) * 16
    planes = torch.full((1, 2, Hkv, lin_rows, D), NAN, dtype=BF16, device="cuda")
    lin_state = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert torch.equal(run((planes, lin_state)), out), f"{name}: the lin= variant differs"
    assert lin_state.tolist() == [L, 1]
