"""The weight-fp4 GEMM (csrc/gemm_wfp4.hip: svlm_gemm_wfp4 / svlm_gemm_wfp4_norm) on every tile / split path, against the fp64 reference
on W' = dequantize_blocks_mxfp4(W4, s) at the per-element bound the bf16 paths are held to (tests/gemm_ref64.py: the kernel feeds
v_mfma_f32_16x16x32_bf16 the bf16 values of W', so c = 32 + ceil(kps / 32) + splits, the bf16 count -- not a new tolerance).

Each case (tests/gemm_wfp4_paths.py) runs on the diagnostic library, under its switches if it forces a plan, and asserts that the plan
reported by svlm_diag_last_gemm_plan (field 1 = 3) equals the Python mirror; an unforced case also runs on the product library, which
must give the same bits.  The split-K workspace is NaN around every call, the output sits in a buffer with sentinel rows and (padded
leading dimensions) sentinel columns.  Then the bf16 twin runs on the same operands, `gemm(A, dequant_fp4(W4, s))` (a forced case
forces the twin's split count too): where its plan has the same live split count and K per split, the two outputs must be EQUAL bit
for bit -- every un-split case is one of these, and the language-model shapes are by construction of the kernel's table; the last
test counts them.  For the 7B-width cases the fp64 reference covers 64 output columns (gemm_wfp4_paths.ref_columns); the twin covers
all of them.

The test prints, per case, whether the bf16 twin had the same K per split, and at the end how many cases were bit-equal to it and the
worst err / bound per generator (1.0 = at the limit)."""
import ctypes

import pytest
import torch

import gemm_paths as G
import gemm_ref64 as R
import gemm_wfp4_paths as P
import helpers as H
from test_gemm_paths_gpu import PLAN_KEYS, _untouched, _view, _ws_tail_is_nan

from streaming_vlm_amd.engine import FP4_PREFILL_OPS
from streaming_vlm_amd.weights import dequantize_blocks_mxfp4

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
U8 = torch.uint8
SEEN = {}            # case id -> dict(equal=bool, unsplit=bool, model=bool)
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    assert all(hasattr(HipOps, m) for m in FP4_PREFILL_OPS)
    return HipOps()


@pytest.fixture(scope="module")
def diag():
    return H.diag_ops()


class Run:
    def __init__(self, case):
        M, N, K, ld = case["M"], case["N"], case["K"], case["ld"]
        self.case = case
        o = P.operands(case["gen"], M, N, K, case["bias"], case["res"] or case["inplace"], swiglu=case["act"] == 4)
        self.Wp = o["Wp"]                                           # W', the matrix the kernel multiplies by
        self.A64 = o["A"]
        self.A, _ = _view(M, K, K + 8 if ld else K, fill=o["A"].cuda())
        self.W4, _ = _view(o["W4"].shape[0], K // 2, K // 2 + 32 if ld else K // 2, dtype=U8, fill=o["W4"].cuda())
        self.s = o["s"].cuda().contiguous()
        self.Wp_dev = self.Wp.cuda()
        self.bias = None if o["bias"] is None else o["bias"].cuda()
        self.res_cpu = o["res"]
        self.norm_w = (G._randn((N,), 5, 0.1).float() + 1).to(BF16).cuda() if case["norm"] else None

    def call(self, ops, twin=False):
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
        if twin:            # the scratch path: dequantise, then the bf16 GEMM
            Wb = ops.dequant_fp4(self.W4.contiguous(), self.s, torch.empty((self.W4.shape[0], c["K"]), dtype=BF16, device="cuda"))
            assert torch.equal(Wb, self.Wp_dev)
            if normed:
                ops.gemm_norm(self.A, Wb, self.norm_w, 1e-6, out, xn, bias=self.bias, residual=res, act=c["act"])
            else:
                ops.gemm(self.A, Wb, bias=self.bias, residual=res, out=out, act=c["act"])
        elif normed:
            ops.gemm_wfp4_norm(self.A, self.W4, self.s, self.norm_w, 1e-6, out, xn, bias=self.bias, residual=res, act=c["act"])
        else:
            ops.gemm_wfp4(self.A, self.W4, self.s, bias=self.bias, residual=res, out=out, act=c["act"])
        torch.cuda.synchronize()
        plan = ops.last_gemm_plan() if hasattr(ops.lib, "svlm_diag_last_gemm_plan") else None
        _untouched(obuf, M, N, c["id"] + " C")
        if normed:
            _untouched(xbuf, M, N, c["id"] + " XN")
        return dict(out=out, xn=xn, plan=plan, ws=ws)


def _check(case, run, r, plan, tag):
    K, N = case["K"], case["N"]
    exact = case["gen"] in ("exact", "rowcol", "blocks")
    cols = P.ref_columns(case)
    Wp, bias, res, out = run.Wp, None if run.bias is None else run.bias.cpu(), run.res_cpu, r["out"]
    if cols is not None:
        ci = torch.tensor(cols)
        wi = torch.cat([ci, ci + N]) if case["act"] == 4 else ci
        Wp, bias = Wp[wi], None if bias is None else bias[wi]
        res = None if res is None else res[:, ci]
        out = out.cpu()[:, ci]
    ref, bound, _, _ = R.reference(run.A64, Wp, bias, res, act=case["act"], c=R.fadds(dict(plan, fp8=0), K),
                                   small_ints=case["gen"] == "exact")
    name = f"{case['id']} {tag}"
    w = R.check(name, out, ref, bound, plan=plan, K=K, swiglu=case["act"] == 4, exact=exact)
    if case["norm"]:
        xr, xb = R.norm_reference(r["out"], run.norm_w, None, 1e-6)
        R.check(name + " norm", r["xn"], xr, xb, plan=plan, K=K)
    return w


@pytest.mark.parametrize("case", P.CASES, ids=[c["id"] for c in P.CASES])
def test_gemm_wfp4_path(case, ops, diag):
    M, N, K = case["M"], case["N"], case["K"]
    run = Run(case)
    want = P.plan_wfp4(M, N, K, act=case["act"], norm=case["norm"] is not None, env=case["force"])
    with H.forced_switches(case["force"] or {}):
        rd = run.call(diag)
    got = {k: rd["plan"][k] for k in PLAN_KEYS}
    assert got == {k: want[k] for k in PLAN_KEYS}, f"reported plan {got} != mirror {want}"
    assert got["fp8"] == 3
    _ws_tail_is_nan(rd, want, M, N, case["id"] + " diag")
    if not case["force"]:
        rp = run.call(ops)
        _ws_tail_is_nan(rp, want, M, N, case["id"] + " product")
        assert torch.equal(rd["out"].view(torch.int16), rp["out"].view(torch.int16)), "diagnostic and product libraries differ with no switch set"
        if case["norm"]:
            assert torch.equal(rd["xn"].view(torch.int16), rp["xn"].view(torch.int16))
    w = _check(case, run, rd, want, "diag")
    # the scratch path on the same operands: same K per split -> same bits.  A forced case asks the bf16 dispatch for the same split
    # count (on its 64-row tiles), so that every un-split case and the forced splits have a twin to be compared with
    twin_env = {}
    if case["force"]:
        twin_env = {"SVLM_GEMM_BM": "64", **({"SVLM_GEMM_SPLITS": case["force"]["SVLM_GEMM_WFP4_SPLITS"]} if "SVLM_GEMM_WFP4_SPLITS" in case["force"] else {})}
    with H.forced_switches(twin_env):
        rt = run.call(diag, twin=True)
    tp = rt["plan"]
    assert tp["fp8"] == 0
    same_k = tp["splits"] == want["splits"] and (want["splits"] == 1 or tp["kps"] == want["kps"])
    if same_k:
        assert torch.equal(rd["out"].view(torch.int16), rt["out"].view(torch.int16)), f"same K per split as the bf16 twin ({tp}), different bits"
        if case["norm"]:
            assert torch.equal(rd["xn"].view(torch.int16), rt["xn"].view(torch.int16))
    SEEN[case["id"]] = dict(equal=same_k, unsplit=want["splits"] == 1, model=any(m + "-" in case["note"] for m in P.MODELS))
    if case["gen"] in ("iid", "spread"):
        WORST[case["gen"]] = max(WORST.get(case["gen"], (0.0, 0.0)), w)
    print(f"[bf16 twin] {tp['bm']} rows s{tp['splits']} kps {tp['kps']}: {'bit-equal' if same_k else 'other K per split, not compared'}; worst so far {WORST}")


def test_bit_equal_cases_were_counted():
    if len(SEEN) != len(P.CASES):          # a partial selection of this file: nothing to count
        return
    eq = [k for k, v in SEEN.items() if v["equal"]]
    print(f"[gemm_wfp4] {len(eq)} of {len(SEEN)} cases had the bf16 twin's K per split and were bit-equal to it; worst err / bound {WORST}")
    assert all(v["equal"] for v in SEEN.values() if v["unsplit"]), "an un-split case was not compared"
    assert all(v["equal"] for v in SEEN.values() if v["model"]), "a language-model shape left the scratch path's K per split"
    assert len(eq) >= sum(v["unsplit"] for v in SEEN.values()) > 0


def _same_values(got, want, what):
    """Every element equal as a NUMBER, and as BITS everywhere but at the -0 codes (code 8), which come out as +0: an output is a sum
    of products that starts from +0, and (+0) + (-0) = +0 in round-to-nearest, from any GEMM, the bf16 one on W' included (the argument
    of tests/test_gemm_wfp8_gpu.py:_same_values)."""
    ne = got.float() != want.float()
    n_bad = int(ne.sum())
    neg_zero = want.view(torch.int16) == -32768
    print(f"[all codes, {what}] {n_bad} of {ne.numel()} values differ; {int((got.view(torch.int16) != want.view(torch.int16)).sum())} bit "
          f"patterns differ (the -0 codes: {int(neg_zero.sum())})")
    if n_bad:
        i = [int(v) for v in ne.nonzero()[0]]
        raise AssertionError(f"{what}: {n_bad} values differ, first at {i}: got {float(got[tuple(i)])!r}, want {float(want[tuple(i)])!r}")
    assert bool(torch.isfinite(got.float()).all())
    diff = got.view(torch.int16) != want.view(torch.int16)
    assert torch.equal(diff, neg_zero), f"{what}: bit patterns differ away from the -0 codes ({int((diff & ~neg_zero).sum())} elements)"
    assert bool((got.view(torch.int16)[neg_zero] == 0).all()) and int(neg_zero.sum()) == got.numel() // 16


def test_every_e2m1_code_at_every_position_is_exact(ops):
    """Code of element (n, k) = (n + k) % 16: every row holds all 16 codes at both nibbles of every byte of a 4-byte fragment read and
    at both swizzle positions.  A = identity, so C[m, n] = W'[n, m] is ONE product: it must be dequantize_blocks_mxfp4's value exactly
    (the sign of a zero aside, see _same_values) under four uniform scale bytes and under one scale byte per (row, block).  This test
    settles the byte and nibble order of v_cvt_scalef32_pk_bf16_fp4 and its exactness on the hardware."""
    K = N = 256
    nib = ((torch.arange(K).view(1, K) + torch.arange(N).view(N, 1)) % 16).to(U8)
    codes = (nib[:, 0::2] | (nib[:, 1::2] << 4)).contiguous()
    A = torch.eye(K, dtype=BF16).cuda()
    for byte in (107, 120, 127, 132):
        s = torch.full((N, K // 32), byte, dtype=U8)
        want = dequantize_blocks_mxfp4(codes, s)
        assert float(want.float().abs().max()) == 6.0 * 2.0 ** (byte - 127)
        _same_values(ops.gemm_wfp4(A, codes.cuda(), s.cuda()).cpu(), want.t().contiguous(), f"scale byte {byte}")
    s = (112 + (7 * torch.arange(N).view(N, 1) + 3 * torch.arange(K // 32).view(1, K // 32)) % 32).to(U8)
    assert len(set(s.flatten().tolist())) == 32
    _same_values(ops.gemm_wfp4(A, codes.cuda(), s.cuda()).cpu(), dequantize_blocks_mxfp4(codes, s).t().contiguous(), "scale byte per (row, block)")


def test_every_refused_argument_is_einval(ops):
    lib, p = ops.lib, lambda t: ctypes.c_void_p(t.data_ptr())
    M, N, K = 70, 128, 256
    A = torch.zeros((M, K + 64), dtype=BF16, device="cuda")
    W4 = torch.zeros((2 * N, K // 2 + 32), dtype=U8, device="cuda")
    s = torch.full((2 * N * (K // 32) + 2,), 127, dtype=U8, device="cuda")
    C = torch.zeros((M, N), dtype=BF16, device="cuda")
    g = torch.ones(N, dtype=BF16, device="cuda")

    def call(K_=K, N_=N, ldw=K // 2 + 32, scale=s, w=W4, lda=K + 64, ldc=N, act=0, res=None, ldr=0, norm=False):
        a = [p(A), lda, p(w), ldw, None if scale is None else p(scale), None, None if res is None else p(res), ldr, p(C), ldc, M, N_, K_, act,
             None, 0]
        if norm:
            return lib.svlm_gemm_wfp4_norm(*a, p(g), None, 1e-6, p(C), N, None)
        return lib.svlm_gemm_wfp4(*a, None)
    for norm in (False, True):
        name = b"svlm_gemm_wfp4"
        assert call(norm=norm) == 0
        for what, kw in (("K % 64 != 0", dict(K_=K + 32)), ("K % 64 != 0", dict(K_=96)), ("N % 4 != 0", dict(N_=126)),
                         ("null scales", dict(scale=None)), ("scales not 2-B aligned", dict(scale=s[1:])),
                         ("ldw % 16 != 0", dict(ldw=K // 2 + 8)), ("ldw < K / 2", dict(ldw=K // 2 - 16)),
                         ("codes not 16-B aligned", dict(w=W4.view(-1)[8:])), ("lda % 8 != 0", dict(lda=K + 4)), ("lda < K", dict(lda=K - 8)),
                         ("ldc < N", dict(ldc=N - 4)), ("ldr % 4 != 0", dict(res=C, ldr=N + 2)), ("unknown activation", dict(act=5))):
            assert call(norm=norm, **kw) == -22, what
            assert name in lib.svlm_last_error(), what
    assert call(N_=124) == 0 and call(N_=124, norm=True) == -22, "the norm needs N % 8 == 0"
    assert call(N_=124, act=4) == -22 and call(act=4) == 0, "SwiGLU needs N % 8 == 0"
    assert call(act=4, res=C, ldr=N) == -22, "SwiGLU takes no residual"
    torch.cuda.synchronize()
    assert b"svlm_gemm_wfp4" in lib.svlm_last_error()
    from streaming_vlm_amd._lib import SvlmError
    with pytest.raises(SvlmError):
        ops.gemm_wfp4(A[:, :96], W4[:N, :48], s[:N * 3].view(N, 3))
