"""weights.py:quantize_blocks_mxfp8 / dequantize_blocks_mxfp8, the host definition of the MXFP8 activation format the row quantiser
svlm_quant_mxfp8 (csrc/gemm_mx.hip) is held to bit for bit (tests/test_gemm_mx_gpu.py runs `boundary_rows` through the kernel).  No GPU."""
import pytest
import torch

from streaming_vlm_amd.weights import dequantize_blocks_mxfp8, quantize_blocks_mxfp8

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn


def _next_bf16(v: float) -> float:
    """The bf16 one step above a positive bf16 v."""
    t = torch.tensor([v], dtype=BF16)
    assert float(t) == v
    return float((t.view(torch.int16) + 1).view(BF16))


def boundary_rows():
    """[R, 64] bf16: per row two blocks built around one boundary of the definition -- amax exactly 448 * 2^j and one bf16 step above
    it, all-zero blocks, blocks below the -117 clamp (bf16 subnormals included), ties of the e4m3 grid, e4m3 subnormals, -0."""
    rows = []

    def row(b0, b1):
        r = torch.zeros(64, dtype=torch.float32)
        r[:len(b0)] = torch.tensor(b0, dtype=torch.float32)
        r[32:32 + len(b1)] = torch.tensor(b1, dtype=torch.float32)
        rows.append(r)
    for j in (-126, -118, -40, -9, -1, 0, 1, 7, 60, 118):
        top = 448.0 * 2.0 ** j
        row([top, -top / 2, top / 448], [_next_bf16(top), top, -top])
    row([], [0.0, -0.0])                                                     # all-zero blocks (one holds a -0)
    row([2.0 ** -110, 2.0 ** -117, -2.0 ** -118], [2.0 ** -120, 2.0 ** -126, -2.0 ** -127, 2.0 ** -133])      # the clamp
    row([1.5 * 2.0 ** -127, 1.75 * 2.0 ** -126, 2.0 ** -126 * 0.75], [2.0 ** -125, 3 * 2.0 ** -128])
    # ties on the e4m3 grid under scale 2^0 (amax 256 = 0.5 * 2^9 -> e = 0): 17 -> 16, 19 -> 20, 34 -> 32, 38 -> 40, ...;
    # second block: e4m3 subnormals (multiples of 2^-9), their ties and the signs of the zeros
    row([256.0, 17.0, 19.0, 34.0, 38.0, -17.0, -19.0, 1.0625, 1.1875, 208.0, 240.0],
        [256.0, 2.0 ** -9, 2.0 ** -10, 1.5 * 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, -2.0 ** -10, -1.5 * 2.0 ** -10, 7 * 2.0 ** -9,
         7.5 * 2.0 ** -9, 2.0 ** -6, 2.0 ** -11, -0.0, -2.0 ** -12])
    x = torch.stack(rows)
    xb = x.to(BF16)
    assert torch.equal(xb.float(), x), "the boundary values are bf16 numbers"
    return xb


def test_scale_bytes_at_448_times_a_power_of_two_and_one_step_above():
    for j in (-126, -118, -40, -9, -1, 0, 1, 7, 60, 118):
        top = 448.0 * 2.0 ** j
        x = torch.zeros((1, 64), dtype=BF16)
        x[0, 3], x[0, 32 + 7] = top, _next_bf16(top)
        q, s = quantize_blocks_mxfp8(x)
        e = max(j, -117)
        assert s.tolist() == [[e + 127, max(j + 1, -117) + 127]], (j, s.tolist())
        if j >= -117:
            assert int(q[0, 3]) == 0x7E, "448 * 2^e is the largest code"          # 0x7E = 448
            assert int(q[0, 39]) == 0x76                                          # 225 * 2^(e + 1) -> 224 = 0x76 (nearest; tie to even)
        assert torch.equal(dequantize_blocks_mxfp8(q, s)[0, 3:4].float(), torch.tensor([top if j >= -117 else float(q[0, 3:4].view(FP8).float()) * 2.0 ** -117]))


def test_no_saturation_and_at_least_half_the_scale_is_used():
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((64, 256), generator=g) * torch.pow(2.0, torch.randint(-100, 100, (64, 8), generator=g).float()).repeat_interleave(32, 1)).to(BF16)
    q, s = quantize_blocks_mxfp8(x)
    assert q.dtype == torch.uint8 and s.dtype == torch.uint8 and tuple(q.shape) == (64, 256) and tuple(s.shape) == (64, 8)
    vals = q.view(FP8).float()
    assert bool(torch.isfinite(vals).all()) and float(vals.abs().max()) <= 448.0
    e = s.to(torch.int32) - 127
    amax = x.float().view(64, 8, 32).abs().amax(dim=2)
    assert bool((amax <= 448.0 * torch.pow(2.0, e.float())).all())
    free = e > -117
    assert bool(free.any()) and bool((amax[free].double() > 224.0 * torch.pow(2.0, e[free].double())).all()), "half the scale unused"
    d = dequantize_blocks_mxfp8(q, s, dtype=torch.float32)
    assert torch.equal(dequantize_blocks_mxfp8(q, s).float(), d), "A' is exactly representable in bf16"
    # round to nearest: the error is at most half an e4m3 step of the element's binade (3 mantissa bits), or half a subnormal step
    step = torch.maximum(torch.pow(2.0, torch.floor(torch.log2(d.abs().clamp_min(1e-45))) - 3), torch.pow(2.0, e.float() - 9).repeat_interleave(32, 1))
    assert bool(((d - x.float()).abs() <= step / 2 * (1 + 2.0 ** -20) + 0).all())


def test_zero_blocks_the_clamp_ties_subnormals_and_minus_zero():
    x = boundary_rows()
    q, s = quantize_blocks_mxfp8(x)
    R = x.shape[0]
    zero, clamp, sub, ties = R - 4, R - 3, R - 2, R - 1
    assert s[zero].tolist() == [127, 127] and q[zero, :32].tolist() == [0] * 32 and q[zero, 32:34].tolist() == [0, 0x80]
    # clamp: block 0 has amax 2^-110 (e = -118 -> -117): 2^-110 / 2^-117 = 128 = 0x70, 2^-117 -> 1.0 = 0x38, -2^-118 -> -0.5 = 0xB0
    assert s[clamp].tolist() == [10, 10] and q[clamp, :3].tolist() == [0x70, 0x38, 0xB0]
    # block 1: 2^-120 -> 2^-3 = 0x20, 2^-126 -> 2^-9 = 0x01, -2^-127 -> a tie between 0 and 2^-9 -> -0, 2^-133 -> 0: toward zero
    assert q[clamp, 32:36].tolist() == [0x20, 0x01, 0x80, 0x00]
    d = dequantize_blocks_mxfp8(q, s).float()
    nz = d[d != 0]
    assert float(nz.abs().min()) >= 2.0 ** -126, "every non-zero A' is a normal bf16"
    assert s[sub].tolist() == [10, 10] and q[sub, :3].tolist() == [0x01, 0x02, 0x01]      # in units of 2^-126: 0.75 -> 1, 1.75 -> 2, 0.75 -> 1
    # ties on the grid (scale 2^0)
    assert s[ties].tolist() == [127, 127]
    v = q[ties].view(FP8).float()
    assert v[:11].tolist() == [256.0, 16.0, 20.0, 32.0, 40.0, -16.0, -20.0, 1.0, 1.25, 208.0, 240.0]
    k = 2.0 ** -9
    assert v[32:46].tolist() == [256.0, k, 0.0, k, 2 * k, 2 * k, -0.0, -k, 7 * k, 8 * k, 8 * k, 0.0, -0.0, -0.0]
    assert q[ties, 32 + 6].item() == 0x80 and q[ties, 32 + 12].item() == 0x80 and q[ties, 32 + 13].item() == 0x80, "the sign of a zero is kept"


def test_non_finite_blocks_are_all_nan_codes_with_scale_127():
    x = torch.ones((2, 96), dtype=BF16)
    x[0, 5], x[1, 64], x[1, 33] = float("inf"), float("nan"), float("-inf")
    q, s = quantize_blocks_mxfp8(x)
    assert s.tolist() == [[127, 119, 119], [119, 127, 127]]
    assert bool((q[0, :32] == 0x7F).all()) and bool((q[1, 32:] == 0x7F).all()) and bool((q[0, 32:] == 0x78).all())      # 1 / 2^-8 = 256 = 0x78
    d = dequantize_blocks_mxfp8(q, s).float()
    assert bool(torch.isnan(d[0, :32]).all()) and bool(torch.isnan(d[1, 32:]).all()) and bool((d[0, 32:] == 1).all())


def test_refused_shapes():
    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_blocks_mxfp8(torch.zeros((4, 48), dtype=BF16))
    with pytest.raises(ValueError, match="multiple of 32"):
        quantize_blocks_mxfp8(torch.zeros((64,), dtype=BF16))
    with pytest.raises(ValueError, match="bf16"):
        quantize_blocks_mxfp8(torch.zeros((4, 64)))


def test_matches_an_independent_division_based_definition():
    """e = the smallest integer with amax <= 448 * 2^e, found by search in fp64; codes by torch's e4m3 cast of x / 2^e."""
    x = boundary_rows()
    g = torch.Generator().manual_seed(5)
    x = torch.cat([x, (torch.randn((40, 64), generator=g) * torch.pow(2.0, torch.randint(-125, 118, (40, 1), generator=g).float())).to(BF16)])
    q, s = quantize_blocks_mxfp8(x)
    for r in range(x.shape[0]):
        for b in range(2):
            blk = x[r, 32 * b:32 * b + 32].double()
            amax = float(blk.abs().max())
            e = 0
            if amax > 0:
                e = -200
                while amax > 448.0 * 2.0 ** e:
                    e += 1
                e = max(e, -117)
            assert int(s[r, b]) == e + 127, (r, b, amax)
            want = (blk / 2.0 ** e).float().to(FP8).view(torch.uint8)
            assert torch.equal(q[r, 32 * b:32 * b + 32], want), (r, b)
