"""The MX prefill kernels (csrc/gemm_mx.hip) on the MI355X.

Row quantiser svlm_quant_mxfp8: codes and scale bytes equal to weights.py:quantize_blocks_mxfp8 bit for bit.

Operand layout of v_mfma_scale_f32_16x16x128_f8f6f4 (`test_every_code_at_every_k_position_is_exact`, the first test to make pass):
every e4m3 byte but the two NaN codes and every e2m1 code at every one of the 128 k positions of a K-step, under five scale patterns
per operand, ONE non-zero product per output, so the expected bf16 value is exact and compared with torch.equal.  It pins which
lanes own which k, the nibble order and which lane's scale byte the hardware applies.

Paths (tests/gemm_mx_paths.py): each case on the diagnostic library with its plan forced, the reported plan (field 1 = 4) against the
mirror, un-forced cases on the product library too with the same bits; NaN workspace, sentinel rows and columns.  Bound: the fp64
reference on (A', W') with c = fadds(dict(plan, fp8=1), K) -- the derived bound the fp8 MFMA is held to (128 products per block):
err / bound <= 1 per element and mean <= MEAN_TOL; the `exact` and `blocks` generators bit-exact."""
import ctypes

import pytest
import torch

import gemm_mx_paths as P
import gemm_paths as G
import gemm_ref64 as R
import helpers as H
from test_gemm_paths_gpu import PLAN_KEYS, _untouched, _view, _ws_tail_is_nan
from test_mxfp8_quant_host import boundary_rows

from streaming_vlm_amd.engine import MX_PREFILL_OPS
from streaming_vlm_amd.weights import dequantize_blocks_mxfp4, dequantize_blocks_mxfp8, quantize_blocks_mxfp8

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
U8 = torch.uint8
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    assert all(hasattr(HipOps, m) for m in MX_PREFILL_OPS)
    return HipOps()


@pytest.fixture(scope="module")
def diag():
    return H.diag_ops()


# ------------------------------------------------------------------------------------------------ the quantiser
def _quant_equal(ops, x, what, pad=False):
    rows, cols = x.shape
    want_q, want_s = quantize_blocks_mxfp8(x)
    xd, _ = _view(rows, cols, cols + 8 if pad else cols, fill=x.cuda())
    q, qbuf = _view(rows, cols, cols + 16 if pad else cols, extra_rows=1, dtype=U8)
    s = torch.full((rows + 1, cols // 32), 0x7F, dtype=U8, device="cuda")
    ops.quant_mxfp8(xd, q, s[:rows])
    torch.cuda.synchronize()
    _untouched(qbuf, rows, cols, what + " codes")
    assert bool((s[rows:] == 0x7F).all()), what + ": scale bytes below the last row were written"
    bad = (s[:rows].cpu() != want_s).nonzero()
    assert not len(bad), f"{what}: {len(bad)} scale bytes differ, first at {bad[0].tolist()}: got {int(s[tuple(bad[0])])}, want {int(want_s[tuple(bad[0])])}"
    bad = (q.cpu() != want_q).nonzero()
    assert not len(bad), (f"{what}: {len(bad)} codes differ, first at {bad[0].tolist()}: x {float(x[tuple(bad[0])])!r} got "
                          f"{int(q[tuple(bad[0])]):#x}, want {int(want_q[tuple(bad[0])]):#x}")


@pytest.mark.parametrize("pad", [False, True], ids=["dense", "padded"])
def test_quantiser_equals_the_host_definition(ops, pad):
    g = torch.Generator().manual_seed(11)
    for rows in (1, 3, 65):
        for cols in (32, 160, 1536):
            x = torch.randn((rows, cols), generator=g)
            # magnitudes spread over 8 decades inside every block
            x = (x * torch.pow(10.0, torch.rand((rows, cols), generator=g) * 8 - 4)).to(BF16)
            _quant_equal(ops, x, f"{rows}x{cols} spread", pad)
    _quant_equal(ops, boundary_rows(), "boundary rows", pad)
    x = torch.randn((3, 160), generator=g).to(BF16)
    x[1, 40], x[2, 159] = float("inf"), float("nan")
    _quant_equal(ops, x, "non-finite blocks", pad)
    q, s = ops.quant_mxfp8(x.cuda())
    assert bool((q[1, 32:64] == 0x7F).all()) and int(s[1, 1]) == 127 and bool((q[2, 128:] == 0x7F).all()) and int(s[2, 4]) == 127


# ------------------------------------------------------------------------------------------------ operand layout of the scaled MFMA
PATTERNS = ("all 127", "one byte per block", "extreme low", "extreme high", "mixed per row")


def _scales(name, rows, nb, a, b):
    """Scale bytes [rows, nb] of one operand; (a, b) make the A and the W bytes of a (row, block) differ.  The extremes keep every
    product a normal fp32 / bf16 number: 2^-66 (smallest e4m3) x 2^-58 (smallest e2m1) and 448 x 2^53 x 6 x 2^53."""
    r, k = torch.arange(rows).view(rows, 1), torch.arange(nb).view(1, nb)
    v = {"all 127": 127 + 0 * (r + k), "one byte per block": 119 + (a * r + b * k) % 17, "extreme low": 70 + (a * r + b * k) % 3,
         "extreme high": 180 - (a * r + b * k) % 3, "mixed per row": 127 + ((a * r) % 7 - 3) * 5 + 0 * k}[name]
    return v.to(U8)


@pytest.mark.parametrize("MN,K", [(16, 128), (32, 128), (16, 256), (32, 256)])
@pytest.mark.parametrize("swept", ["e4m3", "e2m1"])
def test_every_code_at_every_k_position_is_exact(ops, swept, MN, K):
    """One operand is ONE-HOT per row (a 1.0 at k = 16 g + row, group g of the launch), the other is dense with a different code at every
    (row, k), so C[m, n] is one non-zero product and must be the product of the two dequantised values exactly (at most 4 + 2
    significant bits).  e4m3: A8[m, k] = the ((m + t + 3 k) % 254)-th of the 254 non-NaN bytes; over the rows and the batches t every
    byte visits every k.  e2m1: code of W[n, k] = (n + k) % 16, both nibbles of every byte.  Five scale patterns on both operands at
    once (the bytes of A and W differ).  This pins the layout csrc/gemm_mx.hip states: the e2m1 lane group fq owns k = 32 fq .. + 31
    in ascending byte order, the even k in the low nibble; the e4m3 lane group fq owns k = 16 fq .. + 15 and 64 + 16 fq .. + 15; the
    scale of block j (k = 32 j .. + 31) of a row comes from lane group j on either operand."""
    nb = K // 32
    r, k = torch.arange(MN), torch.arange(K)
    e4 = torch.tensor([c for c in range(256) if c not in (0x7F, 0xFF)], dtype=U8)
    seen = torch.zeros((256 if swept == "e4m3" else 16, 128), dtype=torch.bool)
    for pname in PATTERNS:
        sa, sw = _scales(pname, MN, nb, 5, 3), _scales(pname, MN, nb, 7, 2)
        for g in range(K // MN):
            kk = g * MN + r
            for t in (range(0, 254, MN) if swept == "e4m3" else (0,)):
                if swept == "e4m3":
                    A8 = e4[(r.view(MN, 1) + t + 3 * k.view(1, K)) % 254]
                    nibs = torch.zeros((MN, K), dtype=U8)
                    nibs[r, kk] = 2                                            # W[n, kk[n]] = 1.0
                    seen[A8[:, kk].reshape(-1).long(), (kk % 128).repeat(MN)] = True
                else:
                    A8 = torch.zeros((MN, K), dtype=U8)
                    A8[r, kk] = 0x38                                           # A[m, kk[m]] = 1.0
                    nibs = ((r.view(MN, 1) + k.view(1, K)) % 16).to(U8)
                    seen[nibs[:, kk].reshape(-1).long(), (kk % 128).repeat(MN)] = True
                W4 = (nibs[:, 0::2] | (nibs[:, 1::2] << 4)).contiguous()
                Ap, Wp = dequantize_blocks_mxfp8(A8, sa).float(), dequantize_blocks_mxfp4(W4, sw).float()
                if swept == "e4m3":
                    want = Ap[:, kk] * Wp[r, kk].view(1, MN)                   # [m, n] = A'[m, kk[n]] W'[n, kk[n]]
                else:
                    want = Ap[r, kk].view(MN, 1) * Wp[:, kk].t()               # [m, n] = A'[m, kk[m]] W'[n, kk[m]]
                assert torch.equal(want.to(BF16).float(), want) and bool(torch.isfinite(want).all())
                got = ops.gemm_mx_a8w4(A8.cuda(), sa.cuda(), W4.cuda(), sw.cuda()).cpu().float()
                if not torch.equal(got, want):
                    i = [int(v) for v in (got != want).nonzero()[0]]
                    raise AssertionError(f"{swept} sweep, scales '{pname}', group {g}, batch {t}: {int((got != want).sum())} of {got.numel()} "
                                         f"outputs differ, first at {i}: got {float(got[tuple(i)])!r}, want {float(want[tuple(i)])!r}")
    codes = e4.long() if swept == "e4m3" else torch.arange(16)
    assert bool(seen[codes].all()), "a code missed a k position"


# ------------------------------------------------------------------------------------------------ paths
class Run:
    def __init__(self, case):
        M, N, K, ld = case["M"], case["N"], case["K"], case["ld"]
        self.case = case
        o = P.operands(case["gen"], M, N, K, case["bias"], case["res"] or case["inplace"], swiglu=case["act"] == 4)
        self.Ap, self.Wp = o["Ap"], o["Wp"]                       # the matrices the kernel multiplies
        self.A8, _ = _view(M, K, K + 16 if ld else K, dtype=U8, fill=o["A8"].cuda())
        self.W4, _ = _view(o["W4"].shape[0], K // 2, K // 2 + 32 if ld else K // 2, dtype=U8, fill=o["W4"].cuda())
        self.sa, self.s = o["sa"].cuda().contiguous(), o["s"].cuda().contiguous()
        self.bias = None if o["bias"] is None else o["bias"].cuda()
        self.res_cpu = o["res"]
        self.norm_w = (G._randn((N,), 5, 0.1).float() + 1).to(BF16).cuda() if case["norm"] else None

    def call(self, ops):
        c = self.case
        M, N, ld = c["M"], c["N"], c["ld"]
        normed = c["norm"] is not None
        out, obuf = _view(M, N, N + ((8 if normed else 4) if ld else 0), extra_rows=2)
        res = None
        if c["inplace"]:
            out.copy_(self.res_cpu.cuda())
            res = out
        elif self.res_cpu is not None:
            res, _ = _view(M, N, N + 12 if ld else N, fill=self.res_cpu.cuda())
        xn = xbuf = None
        if normed:
            xn, xbuf = _view(M, N, N + 16 if ld else N, extra_rows=2)
        ws = ops._ws(out.device)
        ws.fill_(float("nan"))
        if normed:
            ops.gemm_mx_a8w4_norm(self.A8, self.sa, self.W4, self.s, self.norm_w, 1e-6, out, xn, bias=self.bias, residual=res, act=c["act"])
        else:
            ops.gemm_mx_a8w4(self.A8, self.sa, self.W4, self.s, bias=self.bias, residual=res, out=out, act=c["act"])
        torch.cuda.synchronize()
        plan = ops.last_gemm_plan() if hasattr(ops.lib, "svlm_diag_last_gemm_plan") else None
        _untouched(obuf, M, N, c["id"] + " C")
        if normed:
            _untouched(xbuf, M, N, c["id"] + " XN")
        return dict(out=out, xn=xn, plan=plan, ws=ws)


def _check(case, run, r, plan, tag):
    K, N = case["K"], case["N"]
    exact = case["gen"] in ("exact", "blocks")
    cols = P.ref_columns(case)
    Wp, bias, res, out = run.Wp, None if run.bias is None else run.bias.cpu(), run.res_cpu, r["out"]
    if cols is not None:
        ci = torch.tensor(cols)
        wi = torch.cat([ci, ci + N]) if case["act"] == 4 else ci
        Wp, bias = Wp[wi], None if bias is None else bias[wi]
        res = None if res is None else res[:, ci]
        out = out.cpu()[:, ci]
    ref, bound, _, _ = R.reference(run.Ap, Wp, bias, res, act=case["act"], c=R.fadds(dict(plan, fp8=1), K), small_ints=case["gen"] == "exact")
    name = f"{case['id']} {tag}"
    w = R.check(name, out, ref, bound, plan=plan, K=K, swiglu=case["act"] == 4, exact=exact)
    if case["norm"]:
        xr, xb = R.norm_reference(r["out"], run.norm_w, None, 1e-6)
        R.check(name + " norm", r["xn"], xr, xb, plan=plan, K=K)
    return w


@pytest.mark.parametrize("case", P.CASES, ids=[c["id"] for c in P.CASES])
def test_gemm_mx_path(case, ops, diag):
    M, N, K = case["M"], case["N"], case["K"]
    run = Run(case)
    want = P.plan_mx(M, N, K, act=case["act"], norm=case["norm"] is not None, env=case["force"])
    with H.forced_switches(case["force"] or {}):
        rd = run.call(diag)
    got = {k: rd["plan"][k] for k in PLAN_KEYS}
    assert got == {k: want[k] for k in PLAN_KEYS}, f"reported plan {got} != mirror {want}"
    assert got["fp8"] == 4
    _ws_tail_is_nan(rd, want, M, N, case["id"] + " diag")
    if not case["force"]:
        rp = run.call(ops)
        _ws_tail_is_nan(rp, want, M, N, case["id"] + " product")
        assert torch.equal(rd["out"].view(torch.int16), rp["out"].view(torch.int16)), "diagnostic and product libraries differ with no switch set"
        if case["norm"]:
            assert torch.equal(rd["xn"].view(torch.int16), rp["xn"].view(torch.int16))
    w = _check(case, run, rd, want, "diag")
    if case["gen"] in ("iid", "spread"):
        WORST[case["gen"]] = max(WORST.get(case["gen"], (0.0, 0.0)), w)
    print(f"[gemm_mx] worst err / bound so far {WORST}")


def test_the_case_table_covers_what_it_must():
    forced = [c for c in P.CASES if c["force"]]
    plans = [P.plan_mx(c["M"], c["N"], c["K"], act=c["act"], norm=c["norm"] is not None, env=c["force"]) for c in forced]
    assert {(p["bm"], p["splits"]) for p in plans} >= {(bm, s) for bm in (64, 128) for s in (1, 2, 3)}
    assert {c["M"] for c in forced} >= {1, 17, 33, 129, 290} and {c["N"] for c in forced} >= {128, 132, 264}
    assert {c["K"] for c in forced} >= {128, 384, 1536}
    for bm in ("64", "128"):
        mine = [c for c in forced if c["force"]["SVLM_GEMM_MX_BM"] == bm]
        assert any(c["act"] == 4 for c in mine) and any(c["norm"] for c in mine) and any(c["ld"] for c in mine)
        assert any(c["bias"] for c in mine) and any(c["res"] for c in mine) and any(c["inplace"] for c in mine)
    assert sum(1 for c in P.CASES if "7b-" in c["note"] and c["M"] == 290) == 4 and any(not c["force"] for c in P.CASES)


def test_every_refused_argument_is_einval(ops):
    lib, p = ops.lib, lambda t: ctypes.c_void_p(t.data_ptr())
    M, N, K = 70, 128, 256
    A8 = torch.zeros((M, K + 64), dtype=U8, device="cuda")
    sa = torch.full((M * (K // 32) + 4,), 127, dtype=U8, device="cuda")
    W4 = torch.zeros((2 * N, K // 2 + 32), dtype=U8, device="cuda")
    s = torch.full((2 * N * (K // 32) + 4,), 127, dtype=U8, device="cuda")
    C = torch.zeros((M, N), dtype=BF16, device="cuda")
    g = torch.ones(N, dtype=BF16, device="cuda")

    def call(K_=K, N_=N, ldw=K // 2 + 32, scale=s, a_scale=sa, a=A8, w=W4, lda=K + 64, ldc=N, act=0, res=None, ldr=0, norm=False):
        args = [p(a), lda, None if a_scale is None else p(a_scale), p(w), ldw, None if scale is None else p(scale), None,
                None if res is None else p(res), ldr, p(C), ldc, M, N_, K_, act, None, 0]
        if norm:
            return lib.svlm_gemm_mx_a8w4_norm(*args, p(g), None, 1e-6, p(C), N, None)
        return lib.svlm_gemm_mx_a8w4(*args, None)
    for norm in (False, True):
        assert call(norm=norm) == 0
        for what, kw in (("K % 128 != 0", dict(K_=K + 64)), ("K % 128 != 0", dict(K_=192)), ("N % 4 != 0", dict(N_=126)),
                         ("null W scales", dict(scale=None)), ("null A scales", dict(a_scale=None)),
                         ("W scales not 4-B aligned", dict(scale=s[2:])), ("A scales not 4-B aligned", dict(a_scale=sa[1:])),
                         ("ldw % 16 != 0", dict(ldw=K // 2 + 8)), ("ldw < K / 2", dict(ldw=K // 2 - 16)),
                         ("W codes not 16-B aligned", dict(w=W4.view(-1)[8:])), ("A codes not 16-B aligned", dict(a=A8.view(-1)[8:])),
                         ("lda % 16 != 0", dict(lda=K + 8)), ("lda < K", dict(lda=K - 16)),
                         ("ldc < N", dict(ldc=N - 4)), ("ldr % 4 != 0", dict(res=C, ldr=N + 2)), ("unknown activation", dict(act=5))):
            assert call(norm=norm, **kw) == -22, what
            assert b"svlm_gemm_mx_a8w4" in lib.svlm_last_error(), what
    assert call(N_=124) == 0 and call(N_=124, norm=True) == -22, "the norm needs N % 8 == 0"
    assert call(N_=124, act=4) == -22 and call(act=4) == 0, "SwiGLU needs N % 8 == 0"
    assert call(act=4, res=C, ldr=N) == -22, "SwiGLU takes no residual"
    x = torch.zeros((4, 96), dtype=BF16, device="cuda")
    q = torch.zeros((4, 96), dtype=U8, device="cuda")
    for what, a in (("cols % 32 != 0", (p(x), 96, p(q), 96, p(sa), 4, 80, None)), ("ldx % 8 != 0", (p(x), 94, p(q), 96, p(sa), 4, 64, None)),
                    ("ldq % 16 != 0", (p(x), 96, p(q), 88, p(sa), 4, 64, None)), ("ldx < cols", (p(x), 32, p(q), 96, p(sa), 4, 64, None)),
                    ("null scales", (p(x), 96, p(q), 96, None, 4, 64, None))):
        assert lib.svlm_quant_mxfp8(*a) == -22, what
        assert b"svlm_quant_mxfp8" in lib.svlm_last_error(), what
    assert lib.svlm_quant_mxfp8(p(x), 96, p(q), 96, p(sa), 4, 96, None) == 0
    torch.cuda.synchronize()
    from streaming_vlm_amd._lib import SvlmError
    with pytest.raises(SvlmError):
        ops.gemm_mx_a8w4(A8[:, :192], sa[:M * 6].view(M, 6), W4[:N, :96], s[:N * 6].view(N, 6))
    with pytest.raises(SvlmError):
        ops.quant_mxfp8(x[:, :80])
