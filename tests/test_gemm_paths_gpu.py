"""Every GEMM tile / split path against an fp64 reference (tests/gemm_ref64.py), with the path named in the case id.

The case list, the operand generators and the Python mirror of the dispatch live in tests/gemm_paths.py; tests/test_gemm_ref64.py checks
them without a GPU (coverage of every kernel instantiation, mirror == the library's own plan, injected faults).  Each case here
  1. runs on the DIAGNOSTIC library (-DSVLM_TUNING, built by build() next to the product library) with no switch set and asserts
     that the plan it reports equals the mirror's -- tile rows, waves, ring stages, DMA or register-staged, live splits, K per split,
     table hit, norm fused into the reduce;
  2. runs on the PRODUCT library and asserts bit equality with 1. (diagnostic == product when nothing is forced);
  3. if the case forces a plan: runs on the diagnostic library under the switches, asserts the reported plan equals the forced one
     and checks that output too;
  4. checks the output against the fp64 reference: bit equality for the `exact` and `rowcol` generators, the derived per-element
     bound and the mean bound for `iid` and `spread`.
Around every call the split-K workspace is NaN (a slab element read but never written poisons the output) and must still be NaN
beyond splits * M * N afterwards; the output lives in a buffer with two sentinel rows below M (and, for the leading-dimension cases,
sentinel padding columns: lda = K + 8, ldw = K + 16, ldc = N + 4, ldr = N + 12) that must be bit-identical afterwards.
svlm_gemm_bf16_norm needs 16-byte aligned output rows (ldc % 8 == 0), so its leading-dimension cases use ldc = N + 8, ldxn = N + 16
and assert that ldc = N + 4 is rejected.

Both libraries live in one process (two CDLL handles, each with its own copy of the code object).

Observed on an MI355X (1.0 = at the limit): worst err / bound  iid 0.993 (mean 0.352), spread 0.994 (mean 0.265); exact and rowcol: no
element differs on any path.  A ratio just under 1 is what a derived bound gives: a Linear output that lands next to a rounding tie
errs by the whole half ulp.  160 tests in 19.2 s, the slowest being the fp64 reference of the (590, 18944, 3584) SwiGLU case (2.8 s);
tests/test_attn_merge_gpu.py takes about 10 s.
"""
import pytest
import torch

import gemm_paths as G
import gemm_ref64 as R
import helpers as H

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
SENTINEL = 0x7FC5                     # int16 bit pattern of a bf16 NaN with a payload no kernel produces
PLAN_KEYS = ("fp8", "bm", "waves", "stages", "dma", "splits", "kps", "table", "norm_fused")


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def diag():
    return H.diag_ops()


def _view(rows, cols, ld, extra_rows=0, dtype=BF16, fill=None):
    """(rows, cols) view into a (rows + extra_rows, ld) device buffer pre-filled with the sentinel -> (view, buffer)."""
    if dtype == BF16:
        buf = torch.full((rows + extra_rows, ld), SENTINEL, dtype=torch.int16, device="cuda").view(BF16)
    else:
        buf = torch.full((rows + extra_rows, ld), 0x7F, dtype=torch.uint8, device="cuda").view(dtype)
    v = buf[:rows, :cols]
    if fill is not None:
        v.copy_(fill)
    return v, buf


def _untouched(buf, rows, cols, what):
    """Everything of `buf` outside [:rows, :cols] still holds the sentinel, bit for bit."""
    raw = buf.view(torch.int16) if buf.dtype == BF16 else buf.view(torch.uint8)
    want = SENTINEL if buf.dtype == BF16 else 0x7F
    assert bool((raw[rows:] == want).all()), f"{what}: rows below M were written"
    assert bool((raw[:rows, cols:] == want).all()), f"{what}: padding columns were written"


class Run:
    """Device operands of one case, laid out with or without padded leading dimensions."""

    def __init__(self, case, o, ops):
        M, N, K, ld = case["M"], case["N"], case["K"], case["ld"]
        self.case = case
        fp8 = case["kind"] == "fp8"
        if fp8:
            if case["gen"] in ("exact", "rowcol"):
                a8, w8 = o["A"].cuda().to(FP8), o["W"].cuda().to(FP8)
                sa, sw = torch.ones(M, device="cuda"), torch.ones(N, device="cuda")
            else:
                a8, sa = ops.quant_rows_fp8(o["A"].cuda())
                w8, sw = ops.quant_rows_fp8(o["W"].cuda())
            self.A64, self.W64, self.sa, self.sw = a8.float().cpu(), w8.float().cpu(), sa.cpu(), sw.cpu()
            pa, pw = 16, 32                                # fp8 rows need 16-byte alignment: lda = K + 16, ldw = K + 32
            self.A, _ = _view(M, K, K + pa if ld else K, dtype=FP8, fill=a8)
            self.W, _ = _view(N, K, K + pw if ld else K, dtype=FP8, fill=w8)
            self.sa_d, self.sw_d = sa, sw
        else:
            self.A64, self.W64 = o["A"], o["W"]
            self.A, _ = _view(M, K, K + 8 if ld else K, fill=o["A"].cuda())
            self.W, _ = _view(o["W"].shape[0], K, K + 16 if ld else K, fill=o["W"].cuda())
        self.bias = None if o["bias"] is None else o["bias"].cuda()
        self.res_cpu = o["res"]
        self.norm_w = self.norm_b = None
        if case["norm"]:
            self.norm_w = (G._randn((N,), 5, 0.1).float() + 1).to(BF16).cuda()
            self.norm_b = G._randn((N,), 6, 0.1).cuda() if case["norm"] == "ln" else None

    def call(self, ops):
        """-> dict(out, xn, q8, qs, plan | None); checks sentinels and the workspace."""
        c = self.case
        M, N, K, ld = c["M"], c["N"], c["K"], c["ld"]
        normed = c["norm"] is not None
        ldc = N + ((8 if normed else 4) if ld else 0)
        out, obuf = _view(M, N, ldc, extra_rows=2)
        res = None
        if c["inplace"]:
            out.copy_(self.res_cpu.cuda())
            res = out
        elif self.res_cpu is not None:
            res, _ = _view(M, N, N + 12 if ld else N, fill=self.res_cpu.cuda())
        xn = xbuf = q8 = qs = None
        if normed:
            xn, xbuf = _view(M, N, N + 16 if ld else N, extra_rows=2)
        ws = ops._ws(out.device)
        ws.fill_(float("nan"))
        if c["kind"] == "fp8":
            kw = {}
            if normed:
                kw = dict(norm_w=self.norm_w, norm_b=self.norm_b, out_norm=xn)
                if c["note"] == "normq":
                    q8 = torch.empty((M, N), dtype=FP8, device="cuda")
                    qs = torch.empty((M,), dtype=torch.float32, device="cuda")
                    kw["out_norm_q"] = (q8, qs)
            ops.gemm_fp8(self.A, self.sa_d, self.W, self.sw_d, bias=self.bias, residual=res, out=out, act=c["act"], **kw)
        elif normed:
            ops.gemm_norm(self.A, self.W, self.norm_w, 1e-6, out, xn, bias=self.bias, residual=res, act=c["act"], norm_b=self.norm_b)
        else:
            ops.gemm(self.A, self.W, bias=self.bias, residual=res, out=out, act=c["act"])
        torch.cuda.synchronize()
        plan = ops.last_gemm_plan() if hasattr(ops.lib, "svlm_diag_last_gemm_plan") else None
        _untouched(obuf, M, N, c["id"] + " C")
        if normed:
            _untouched(xbuf, M, N, c["id"] + " XN")
        return dict(out=out, xn=xn, q8=q8, qs=qs, plan=plan, ws=ws)


def _ws_tail_is_nan(r, plan, M, N, what):
    used = plan["splits"] * M * N if plan["splits"] > 1 else 0
    assert bool(torch.isnan(r["ws"][used:]).all()), f"{what}: the workspace beyond splits * M * N was written"


def _check(case, run, r, plan, ops_for_quant, tag):
    M, N, K = case["M"], case["N"], case["K"]
    exact = case["gen"] in ("exact", "rowcol")
    kw = dict(a_scale=run.sa, w_scale=run.sw) if case["kind"] == "fp8" else {}
    res = run.res_cpu
    ref, bound, _, _ = R.reference(run.A64, run.W64, None if run.bias is None else run.bias.cpu(), res, act=case["act"],
                                   c=R.fadds(plan, K), small_ints=exact, **kw)
    if exact:
        assert float(ref.abs().max()) <= 256
    name = f"{case['id']} {tag}"
    w = R.check(name, r["out"], ref, bound, plan=plan, K=K, swiglu=case["act"] == 4, exact=exact)
    if case["norm"]:
        xr, xb = R.norm_reference(r["out"], run.norm_w, run.norm_b, 1e-6)
        R.check(name + " norm", r["xn"], xr, xb, plan=plan, K=K)
        if r["q8"] is not None:
            # the fused quantisation against the oracle's CPU recipe (scale = row amax / 448, e4m3 round-to-nearest) applied to the
            # kernel's own normalised rows: codes and scales bit for bit
            from oracle import model as om
            qr, sr = om.quant_rows_fp8(r["xn"].detach().cpu().contiguous())
            assert torch.equal(r["qs"].cpu(), sr.reshape(-1)), name + ": fused quantisation scales"
            assert torch.equal(r["q8"].cpu().view(torch.uint8), qr.to(FP8).view(torch.uint8)), name + ": fused quantisation codes"
    return w


WORST = {}


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_gemm_path(case, ops, diag):
    M, N, K = case["M"], case["N"], case["K"]
    o = G.operands(case["gen"], M, N, K, case["bias"], case["res"] or case["inplace"], swiglu=case["act"] == 4)
    run = Run(case, o, ops)
    want = G.plan_of(case)
    with H.forced_switches({}):
        rd = run.call(diag)
    got = {k: rd["plan"][k] for k in PLAN_KEYS}
    assert got == {k: want[k] for k in PLAN_KEYS}, f"reported plan {got} != mirror {want}"
    _ws_tail_is_nan(rd, want, M, N, case["id"] + " diag")
    rp = run.call(ops)
    _ws_tail_is_nan(rp, want, M, N, case["id"] + " product")
    assert torch.equal(rd["out"].view(torch.int16), rp["out"].view(torch.int16)), "diagnostic and product libraries differ with no switch set"
    if case["norm"]:
        assert torch.equal(rd["xn"].view(torch.int16), rp["xn"].view(torch.int16))
    w = _check(case, run, rp, want, ops, "product")
    if case["force"]:
        wantf = G.plan_of(case, forced=True)
        with H.forced_switches(case["force"]):
            rf = run.call(diag)
        gotf = {k: rf["plan"][k] for k in PLAN_KEYS}
        assert gotf == {k: wantf[k] for k in PLAN_KEYS}, f"forced: reported plan {gotf} != {wantf}"
        _ws_tail_is_nan(rf, wantf, M, N, case["id"] + " forced")
        w = max(w, _check(case, run, rf, wantf, ops, "forced " + wantf["kernel"]))
    WORST[case["gen"]] = max(WORST.get(case["gen"], (0.0, 0.0)), w)
    print(f"[worst so far] {WORST}")


def test_forcing_192_rows_is_reported_as_192_rows(diag, ops):
    """Not vacuous: the switch reaches the dispatch (the product library would ignore it) and the note says so."""
    A, W = G._randn((300, 1024), 1).cuda(), G._randn((260, 1024), 2, 0.05).cuda()
    with H.forced_switches({"SVLM_GEMM_BM": "192"}):
        a = diag.gemm(A, W)
        p = diag.last_gemm_plan()
        b = ops.gemm(A, W)                      # the product library under the same environment: unmoved
    assert p["bm"] == 192 and p["waves"] == 4 and p["stages"] == 3 and p["dma"] == 1, p
    with H.forced_switches({}):
        diag.gemm(A, W)
        assert diag.last_gemm_plan()["bm"] == 64
    assert torch.equal(b, ops.gemm(A, W))
    with pytest.raises(Exception, match="plan note"):
        ops.last_gemm_plan()
    # the 8-wave 128-row force can be switched on and off inside one process
    for on in (True, False, True):
        with H.forced_switches({"SVLM_GEMM_BM": "128", **({"SVLM_GEMM_W8": "1"} if on else {})}):
            diag.gemm(A, W)
            assert diag.last_gemm_plan()["waves"] == (8 if on else 4)
    del a


def test_gemm_norm_rejects_unaligned_output_rows(ops):
    from streaming_vlm_amd._lib import SvlmError
    M, N, K = 70, 256, 1024
    A, W, g = G._randn((M, K), 1).cuda(), G._randn((N, K), 2, 0.05).cuda(), G._randn((N,), 5).cuda()
    out, _ = _view(M, N, N + 4)
    xn, _ = _view(M, N, N + 16)
    with pytest.raises(SvlmError):
        ops.gemm_norm(A, W, g, 1e-6, out, xn)
