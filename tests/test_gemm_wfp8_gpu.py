"""The weight-fp8 GEMM (csrc/gemm_wfp8.hip: svlm_gemm_wfp8 / svlm_gemm_wfp8_norm) on every tile / split path, against the fp64 reference
on W' = dequantize_rows_fp8(W8, s) at the per-element bound the bf16 paths are held to (tests/gemm_ref64.py: the kernel feeds
v_mfma_f32_16x16x32_bf16 the bf16 values of W', so c = 32 + ceil(kps / 32) + splits, the bf16 count).

Each case (tests/gemm_wfp8_paths.py) runs on the diagnostic library, under its switches if it forces a plan, and asserts that the plan
reported by svlm_diag_last_gemm_plan (field 1 = 2) equals the Python mirror; an unforced case also runs on the product library, which
must give the same bits.  The split-K workspace is NaN around every call, the output sits in a buffer with sentinel rows and (padded
leading dimensions) sentinel columns.  Then the bf16 twin runs on the same operands, `gemm(A, dequant_fp8(W8, s))` (a forced case forces the twin's split count too): where its plan has
the same live split count and K per split, the two outputs must be EQUAL bit for bit -- every un-split case is one of these, and the
language-model shapes are by construction of the kernel's table; the last test counts them.

The test prints, per case, whether the bf16 twin had the same K per split, and at the end how many cases were bit-equal to it and the
worst err / bound per generator (1.0 = at the limit)."""
import ctypes

import pytest
import torch

import gemm_paths as G
import gemm_ref64 as R
import gemm_wfp8_paths as P
import helpers as H
from test_gemm_paths_gpu import PLAN_KEYS, _untouched, _view, _ws_tail_is_nan

from streaming_vlm_amd.weights import dequantize_rows_fp8, quantize_rows_fp8_pow2

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
SEEN = {}            # case id -> dict(equal=bool | None, unsplit=bool)
WORST = {}


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def diag():
    return H.diag_ops()


class Run:
    def __init__(self, case):
        M, N, K, ld = case["M"], case["N"], case["K"], case["ld"]
        self.case = case
        o = G.operands(case["gen"], M, N, K, case["bias"], case["res"] or case["inplace"], swiglu=case["act"] == 4)
        q, s = quantize_rows_fp8_pow2(o["W"].cuda())
        self.Wp = dequantize_rows_fp8(q, s).cpu()                   # W', the matrix the kernel multiplies by
        if case["gen"] == "exact":
            assert torch.equal(self.Wp, o["W"]), "0/1 weights survive the quantiser"
        self.A64 = o["A"]
        self.A, _ = _view(M, K, K + 8 if ld else K, fill=o["A"].cuda())
        self.W8, _ = _view(q.shape[0], K, K + 32 if ld else K, dtype=FP8, fill=q)
        self.s = s.contiguous()
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
            Wb = ops.dequant_fp8(self.W8.contiguous(), self.s, torch.empty(tuple(self.W8.shape), dtype=BF16, device="cuda"))
            assert torch.equal(Wb, self.Wp_dev)
            if normed:
                ops.gemm_norm(self.A, Wb, self.norm_w, 1e-6, out, xn, bias=self.bias, residual=res, act=c["act"])
            else:
                ops.gemm(self.A, Wb, bias=self.bias, residual=res, out=out, act=c["act"])
        elif normed:
            ops.gemm_wfp8_norm(self.A, self.W8, self.s, self.norm_w, 1e-6, out, xn, bias=self.bias, residual=res, act=c["act"])
        else:
            ops.gemm_wfp8(self.A, self.W8, self.s, bias=self.bias, residual=res, out=out, act=c["act"])
        torch.cuda.synchronize()
        plan = ops.last_gemm_plan() if hasattr(ops.lib, "svlm_diag_last_gemm_plan") else None
        _untouched(obuf, M, N, c["id"] + " C")
        if normed:
            _untouched(xbuf, M, N, c["id"] + " XN")
        return dict(out=out, xn=xn, plan=plan, ws=ws)


def _check(case, run, r, plan, tag):
    K = case["K"]
    exact = case["gen"] in ("exact", "rowcol")
    ref, bound, _, _ = R.reference(run.A64, run.Wp, None if run.bias is None else run.bias.cpu(), run.res_cpu, act=case["act"],
                                   c=R.fadds(dict(plan, fp8=0), K), small_ints=exact and case["gen"] == "exact")
    name = f"{case['id']} {tag}"
    w = R.check(name, r["out"], ref, bound, plan=plan, K=K, swiglu=case["act"] == 4, exact=exact)
    if case["norm"]:
        xr, xb = R.norm_reference(r["out"], run.norm_w, None, 1e-6)
        R.check(name + " norm", r["xn"], xr, xb, plan=plan, K=K)
    return w


@pytest.mark.parametrize("case", P.CASES, ids=[c["id"] for c in P.CASES])
def test_gemm_wfp8_path(case, ops, diag):
    M, N, K = case["M"], case["N"], case["K"]
    run = Run(case)
    want = P.plan_wfp8(M, N, K, act=case["act"], norm=case["norm"] is not None, env=case["force"])
    with H.forced_switches(case["force"] or {}):
        rd = run.call(diag)
    got = {k: rd["plan"][k] for k in PLAN_KEYS}
    assert got == {k: want[k] for k in PLAN_KEYS}, f"reported plan {got} != mirror {want}"
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
        twin_env = {"SVLM_GEMM_BM": "64", **({"SVLM_GEMM_SPLITS": case["force"]["SVLM_GEMM_WFP8_SPLITS"]} if "SVLM_GEMM_WFP8_SPLITS" in case["force"] else {})}
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
    print(f"[gemm_wfp8] {len(eq)} of {len(SEEN)} cases had the bf16 twin's K per split and were bit-equal to it; worst err / bound {WORST}")
    assert all(v["equal"] for v in SEEN.values() if v["unsplit"]), "an un-split case was not compared"
    assert all(v["equal"] for v in SEEN.values() if v["model"]), "a language-model shape left the scratch path's K per split"
    assert len(eq) >= sum(v["unsplit"] for v in SEEN.values()) > 0


def _same_values(got, want, what):
    """Every element equal as a NUMBER.  The sign of a zero is not compared: an output is a sum of 256 products that starts from +0, and
    (+0) + (-0) = +0 in round-to-nearest, so code 0x80 (-0) comes out as +0 from any GEMM, the bf16 one on W' included."""
    ne = got.float() != want.float()
    n_bad = int(ne.sum())
    bits = int((got.view(torch.int16) != want.view(torch.int16)).sum())
    print(f"[all codes, {what}] {n_bad} of {ne.numel()} values differ; {bits} bit patterns differ (the -0 codes: {int(((want == 0) & (want.view(torch.int16) != 0)).sum())})")
    if n_bad:
        i = [int(v) for v in ne.nonzero()[0]]
        raise AssertionError(f"{what}: {n_bad} values differ, first at {i}: got {float(got[tuple(i)])!r}, want {float(want[tuple(i)])!r}")
    assert bool(torch.isfinite(got.float()).all())
    # ... and as BITS everywhere but at the -0 codes, which come out as +0
    diff = got.view(torch.int16) != want.view(torch.int16)
    neg_zero = want.view(torch.int16) == -32768
    assert torch.equal(diff, neg_zero), f"{what}: bit patterns differ away from the -0 codes ({int((diff & ~neg_zero).sum())} elements)"
    assert bool((got.view(torch.int16)[neg_zero] == 0).all()) and int(neg_zero.sum()) == got.shape[0]


def test_all_finite_e4m3_codes_under_four_scales_are_exact(ops):
    """W8[n, k] = code (k + n) mod 256 (the two NaN codes zeroed): all 254 finite codes, subnormals and -0 included, at every byte
    position of the 8-byte fragment reads and every swizzle position.  A = identity, so C[m, n] = W'[n, m] is ONE product: it must be
    dequantize_rows_fp8's value exactly, for every row scale (the sign of a zero aside, see _same_values)."""
    K = N = 256
    codes = ((torch.arange(K).view(1, K) + torch.arange(N).view(N, 1)) % 256).to(torch.uint8)
    codes[(codes == 0x7F) | (codes == 0xFF)] = 0
    q = codes.view(FP8)
    assert len(set(q.float().flatten().tolist())) == 253            # 254 codes, +0 == -0
    A = torch.eye(K, dtype=BF16).cuda()
    for e in (-20, -7, 0, 5):
        s = torch.full((N,), 2.0 ** e)
        want = dequantize_rows_fp8(q, s)
        assert torch.equal(want.float(), q.float() * s[:, None])
        _same_values(ops.gemm_wfp8(A, q.cuda(), s.cuda()).cpu(), want.t().contiguous(), f"scale 2^{e}")
    # one scale per row, all four at once
    s = torch.tensor([2.0 ** (-20, -7, 0, 5)[n % 4] for n in range(N)])
    _same_values(ops.gemm_wfp8(A, q.cuda(), s.cuda()).cpu(), dequantize_rows_fp8(q, s).t().contiguous(), "four scales")


def test_bad_k_null_scale_and_unaligned_ldw_are_einval(ops):
    lib, p = ops.lib, lambda t: ctypes.c_void_p(t.data_ptr())
    M, N, K = 70, 128, 256
    A = torch.zeros((M, K + 64), dtype=BF16, device="cuda")
    W8 = torch.zeros((N, K + 64), dtype=torch.uint8, device="cuda")
    s = torch.ones(N, device="cuda")
    C = torch.zeros((M, N), dtype=BF16, device="cuda")
    g = torch.ones(N, dtype=BF16, device="cuda")

    def call(K_=K, ldw=K + 64, scale=s, w=W8, norm=False):
        a = [p(A), K + 64, p(w), ldw, None if scale is None else p(scale), None, None, 0, p(C), N, M, N, K_, 0, None, 0]
        if norm:
            return lib.svlm_gemm_wfp8_norm(*a, p(g), None, 1e-6, p(C), N, None)
        return lib.svlm_gemm_wfp8(*a, None)
    for norm in (False, True):
        assert call(norm=norm) == 0
        assert call(K_=K + 32, norm=norm) == -22, "K % 64 != 0"
        assert call(K_=96, norm=norm) == -22
        assert call(scale=None, norm=norm) == -22
        assert call(ldw=K + 8, norm=norm) == -22, "ldw % 16 != 0"
        assert call(w=W8.view(-1)[8:], norm=norm) == -22, "codes not 16-B aligned"
    torch.cuda.synchronize()
    assert b"svlm_gemm_wfp8" in lib.svlm_last_error()
    from streaming_vlm_amd._lib import SvlmError
    with pytest.raises(SvlmError):
        ops.gemm_wfp8(A[:, :96], W8[:, :96].view(FP8), s)
