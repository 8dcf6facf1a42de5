"""CPU self-check of the fp64 attention reference (tests/attn_ref64.py) that the split / merge GPU tests hold the kernels to:
it agrees with the oracle's flash attention within the bf16 bound, and it meets closed forms exactly."""
import math

import torch

from attn_ref64 import attend64, bound_ratios
from oracle import model as om

BF16 = torch.bfloat16
SCALE = 1 / math.sqrt(128)


def _rnd(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF16)


def test_attend64_matches_the_oracle_within_the_bf16_bound():
    """oracle.model.flash_attention rounds P and the output to bf16, as the kernels do: it must sit inside the same per-element
    bound the GPU tests use, for decode (no mask) and for a causal prefill chunk, with GQA groups of 1, 3 and 6."""
    for Hq, Hkv, T, L, off, seed in [(12, 2, 1, 700, None, 0), (6, 2, 37, 300, 263, 1), (4, 4, 64, 64, 0, 2), (6, 1, 5, 2000, 1995, 3)]:
        q, K, V = _rnd((Hq, T, 128), seed), _rnd((Hkv, L, 128), seed + 10), _rnd((Hkv, L, 128), seed + 20)
        ref, E = attend64(q, K, V, off, SCALE)
        G = Hq // Hkv
        want = om.flash_attention(q, K.repeat_interleave(G, 0), V.repeat_interleave(G, 0), off, SCALE)
        ratio, mean = bound_ratios(want, ref, E)
        assert float(ratio.max()) <= 1.0 and mean <= 1.0, (Hq, Hkv, T, L, float(ratio.max()), mean)
        # and the bound is not vacuous: the oracle differs from the fp64 result, by a small fraction of the bound on average
        assert float(ratio.max()) > 0.0 and float(ratio.mean()) < 0.25


def test_attend64_zero_query_is_the_mean_of_the_visible_values():
    Hq, Hkv, T, L, off = 4, 2, 9, 50, 41
    q = torch.zeros((Hq, T, 128), dtype=BF16)
    K, V = _rnd((Hkv, L, 128), 5), _rnd((Hkv, L, 128), 6)
    out, E = attend64(q, K, V, off, SCALE)
    Vd = V.double()
    for h in range(Hq):
        for t in range(T):
            vis = Vd[h // 2, :off + t + 1]
            torch.testing.assert_close(out[h, t], vis.mean(0), rtol=0, atol=1e-12)
            torch.testing.assert_close(E[h, t], vis.abs().mean(0), rtol=0, atol=1e-12)
    out_full, _ = attend64(q[:, :1], K, V, None, SCALE)
    torch.testing.assert_close(out_full[:, 0], Vd.mean(1).repeat_interleave(2, 0), rtol=0, atol=1e-12)


def test_attend64_one_key_far_above_the_rest_gives_its_value_row():
    Hq, Hkv, L = 6, 3, 400
    u = torch.ones(128)
    q = (u + 0.05 * torch.randn(128, generator=torch.Generator().manual_seed(7)))[None, None, :].repeat(Hq, 1, 1).to(BF16)
    K = (0.25 * torch.randn((Hkv, L, 128), generator=torch.Generator().manual_seed(8)))
    K[:, 123] = 200.0 / (128 * SCALE)                                # score ~200 nats above every other key
    K = K.to(BF16)
    V = _rnd((Hkv, L, 128), 9)
    out, E = attend64(q, K, V, None, SCALE)
    for h in range(Hq):
        assert torch.equal(out[h, 0], V[h // 2, 123].double())
        assert torch.equal(E[h, 0], V[h // 2, 123].double().abs())
    # the reference works in relative terms only: every score ~200 nats below zero changes nothing
    out_low, _ = attend64(q, (K.float() - 200.0 / (128 * SCALE)).to(BF16), V, None, SCALE)
    assert torch.isfinite(out_low).all()


def test_attend64_causal_rows_see_exactly_their_prefix():
    Hq, Hkv, T, L = 4, 1, 12, 40
    off = L - T
    q, K, V = _rnd((Hq, T, 128), 11), _rnd((Hkv, L, 128), 12), _rnd((Hkv, L, 128), 13)
    out, E = attend64(q, K, V, off, SCALE)
    for t in range(T):
        o_t, e_t = attend64(q[:, t:t + 1], K[:, :off + t + 1], V[:, :off + t + 1], None, SCALE)
        torch.testing.assert_close(out[:, t], o_t[:, 0], rtol=1e-13, atol=1e-13)
        torch.testing.assert_close(E[:, t], e_t[:, 0], rtol=1e-13, atol=1e-13)
    # keys a row cannot see do not move it, whatever they hold
    K2, V2 = K.clone(), V.clone()
    K2[:, off + 3:] = 50.0
    V2[:, off + 3:] = -7.0
    out2, _ = attend64(q, K2, V2, off, SCALE)
    assert torch.equal(out2[:, :3], out[:, :3])
    assert not torch.allclose(out2[:, 3:], out[:, 3:])
