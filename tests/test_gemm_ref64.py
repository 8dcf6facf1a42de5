"""CPU checks of the GEMM path test machinery (no GPU): the fp64 reference and bound of tests/gemm_ref64.py against the bf16 CPU
oracle and against injected faults, the dispatch mirror of tests/gemm_paths.py against the diagnostic library's own host-side plan,
the coverage conditions of the case list, and the rule that no test sets a tuning switch the product library cannot see."""
import ctypes
import os
import re

import pytest
import torch

import gemm_paths as G
import gemm_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BF16 = torch.bfloat16


def _oracle(o, act=0):
    from ref_ops import RefOps
    return RefOps().gemm(o["A"], o["W"], o["bias"], o["res"], act=act)


@pytest.mark.parametrize("M,N,K,gen,bias,res", [(70, 132, 72, "iid", True, False), (129, 260, 1176, "iid", False, True),
                                                (64, 256, 4096, "spread", True, True), (33, 132, 512, "exact", True, True),
                                                (40, 388, 1984, "rowcol", False, False)])
def test_cpu_oracle_is_within_the_bound(M, N, K, gen, bias, res):
    """No activation: the oracle (F.linear in bf16, fp32 accumulation inside) makes the kernel's roundings -- the Linear output and the
    residual sum.  c: one fp32 addition per product at the very most (a sequential sum)."""
    o = G.operands(gen, M, N, K, bias, res)
    ref, bound, _, _ = R.reference(o["A"], o["W"], o["bias"], o["res"], c=K + 1, small_ints=gen in ("exact", "rowcol"))
    R.check(f"oracle {gen} {M}x{N}x{K}", _oracle(o), ref, bound, exact=gen in ("exact", "rowcol"))


def _plan(K, splits):
    kps = (((K + splits - 1) // splits + 63) // 64) * 64 if splits > 1 else K
    return dict(fp8=0, bm=64, splits=(K + kps - 1) // kps, kps=kps)


@pytest.mark.parametrize("M,N,K,splits", [(70, 132, 1176, 2), (333, 388, 1984, 3), (64, 260, 4096, 8), (193, 256, 18944, 8), (33, 132, 72, 1)])
def test_injected_faults_are_caught_exactly_by_the_exact_generator(M, N, K, splits):
    """One k-column of one split zeroed in A, one 16-row output fragment shifted by a row, one split's partial added twice: each
    changes an integer of the `exact` output at every K, so bit equality fails."""
    o = G.operands("exact", M, N, K, True, True)
    p = _plan(K, splits)
    ref, bound, _, _ = R.reference(o["A"], o["W"], o["bias"], o["res"], c=R.fadds(p, K), small_ints=True)
    assert float(ref.abs().max()) <= 256
    good = _oracle(o)
    R.check("exact clean", good, ref, bound, plan=p, K=K, exact=True)
    k0 = (p["splits"] - 1) * p["kps"]                          # the last split (the one with the tail)
    A2 = o["A"].clone()
    A2[:, k0 + 5] = 0                                           # fault 1: one k-column of one split
    with pytest.raises(AssertionError, match="differ"):
        R.check("exact k-column", _oracle(dict(o, A=A2)), ref, bound, plan=p, K=K, exact=True)
    bad = good.clone()
    bad[16:32] = good[15:31]                                    # fault 2: one 16-row fragment shifted by one row
    with pytest.raises(AssertionError, match="16-row fragments \\[1\\]"):
        R.check("exact shifted fragment", bad, ref, bound, plan=p, K=K, exact=True)
    part = (o["A"][:, k0:].float() @ o["W"][:, k0:].float().t())
    with pytest.raises(AssertionError, match="differ"):        # fault 3: the last split's partial counted twice
        R.check("exact doubled split", (good.float() + part).to(BF16), ref, bound, plan=p, K=K, exact=True)


@pytest.mark.parametrize("M,N,K,splits", [(70, 132, 72, 1), (129, 260, 1176, 2), (333, 388, 1984, 3)])
def test_injected_faults_are_caught_by_the_bound_with_iid_operands(M, N, K, splits):
    """iid operands: the k-column fault is required where ONE product |a w| exceeds the bound of its element (short K; at K = 18944 the
    fp32 term legitimately hides one product, which is what the exact generator is for): computed here, not assumed."""
    o = G.operands("iid", M, N, K, True, False)
    p = _plan(K, splits)
    ref, bound, _, _ = R.reference(o["A"], o["W"], o["bias"], None, c=R.fadds(p, K))
    good = _oracle(o)
    R.check("iid clean (oracle sums sequentially at worst)", good, *R.reference(o["A"], o["W"], o["bias"], None, c=K + 1)[:2])
    k = (p["splits"] - 1) * p["kps"] + 5
    prod = (o["A"][:, k].double()[:, None] * o["W"][:, k].double()[None, :]).abs()
    assert bool((prod > 2 * bound).any()), "pick a shape where one product is visible"
    A2 = o["A"].clone()
    A2[:, k] = 0
    with pytest.raises(AssertionError, match="over the bound"):
        R.check("iid k-column", _oracle(dict(o, A=A2)), ref, bound, plan=p, K=K)
    bad = good.clone()
    bad[16:32] = good[15:31]
    with pytest.raises(AssertionError, match="16-row fragments \\[1\\]"):
        R.check("iid shifted fragment", bad, ref, bound, plan=p, K=K)
    k0 = (p["splits"] - 1) * p["kps"]
    part = o["A"][:, k0:].float() @ o["W"][:, k0:].float().t()
    with pytest.raises(AssertionError, match="over the bound"):
        R.check("iid doubled split", (good.float() + part).to(BF16), ref, bound, plan=p, K=K)
    # a systematic error of 0.65 roundings on every element stays under the per-element bound and fails the mean
    with pytest.raises(AssertionError, match="mean err/bound"):
        R.check("iid systematic", (ref + 0.65 * bound), ref, bound, plan=p, K=K)


def test_activation_bounds_hold_for_the_oracle_roundings():
    """silu / gelu / quick_gelu / SwiGLU: values rounded as common.h's apply_act rounds them, computed here in fp64 + explicit bf16
    roundings from the fp64 Linear output, sit inside the derived bound."""
    rb = lambda t: t.to(BF16).double()
    o = G.operands("spread", 96, 260, 256, True, True, swiglu=False)
    for act in (1, 2, 3):
        ref, bound, z, _ = R.reference(o["A"], o["W"], o["bias"], o["res"], act=act, c=40)
        zb = rb(z)
        if act == 1:
            a = rb(zb * rb(torch.sigmoid(rb(1.702 * zb))))
        elif act == 2:
            a = rb(0.5 * zb * (1 + torch.erf(zb / 2 ** 0.5)))
        else:
            a = rb(zb * torch.sigmoid(zb))
        R.check(f"act {act}", rb(a + o["res"].double()), ref, bound)
    o = G.operands("iid", 96, 132, 256, True, False, swiglu=True)
    ref, bound, z, _ = R.reference(o["A"], o["W"], o["bias"], None, act=4, c=40)
    zb = rb(z)
    R.check("swiglu", rb(rb(zb[:, :132] * torch.sigmoid(zb[:, :132])) * zb[:, 132:]), ref, bound)


# ------------------------------------------------------------------------------------------------ the mirror and the case list
def _diag_lib():
    from streaming_vlm_amd import _lib
    assert os.path.exists(_lib.DIAG_LIB_PATH), (f"{_lib.DIAG_LIB_PATH} is missing: build it with "
                                                "`python -c \"import __graft_entry__ as g; g.build()\"` at the repository root")
    return _lib.load(_lib.DIAG_LIB_PATH)


def _host_plan(lib, case, env):
    """The diagnostic library notes (tile rows, splits, K per split, table hit) before it touches the device, so the call below pins the
    mirror without a GPU: it fails at its first device call (or, on a GPU machine, is never made: see the skip)."""
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("SVLM_GEMM")}
    try:
        os.environ.update(env or {})          # goes to the C environment the diagnostic library reads
        M, N, K = case["M"], case["N"], case["K"]
        fake = ctypes.c_void_p(4096)
        v = (ctypes.c_int * 10)()
        lib.svlm_diag_last_gemm_plan(v, 10)
        seq = v[0]
        if case["kind"] == "fp8":
            nw = fake if case["norm"] else None
            lib.svlm_gemm_fp8(fake, K, fake, fake, K, fake, None, None, 0, fake, N, M, N, K, case["act"], fake, G.WS_BYTES, nw, None, 1e-6,
                              fake if nw else None, N, None)
        else:
            lib.svlm_gemm_bf16(fake, K, fake, K, None, None, 0, fake, N, M, N, K, case["act"], fake, G.WS_BYTES, None)
        lib.svlm_diag_last_gemm_plan(v, 10)
        assert v[0] == seq + 1, f"the call was rejected before it planned: {lib.svlm_last_error()}"
        return dict(fp8=v[1], bm=v[2], splits=v[6], kps=v[7], table=v[8])
    finally:
        for k in (env or {}):
            os.environ.pop(k, None)
        os.environ.update(saved)


def test_mirror_matches_the_library_plan():
    if torch.cuda.is_available():
        pytest.skip("GPU present: the GPU cases assert the reported plan of real launches instead")
    lib = _diag_lib()
    n = 0
    for case in G.CASES:
        for forced in ((False, True) if case["force"] else (False,)):
            want = G.plan_of(case, forced)
            got = _host_plan(lib, case, case["force"] if forced else None)
            assert got == {k: want[k] for k in got}, (case["id"], forced, got, want)
            n += 1
    # and over a grid of shapes no case uses: cost model, table buckets, large-M rules
    case = dict(kind="bf16", act=0, norm=None, force=None)
    for K in (72, 1000, 1176, 1280, 2048, 2056, 3584, 5120, 8960, 18944):
        for M in (1, 64, 65, 193, 256, 257, 290, 384, 385, 590, 1024, 2047, 2048, 2305, 4096):
            for N in (132, 1280, 1536, 3584, 3840, 5120, 6276, 18944):
                c = dict(case, M=M, N=N, K=K)
                want, got = G.plan_of(c), _host_plan(lib, c, None)
                assert got == {k: want[k] for k in got}, (M, N, K, got, want)
                n += 1
    # every tuned-table entry across its row bucket and one bucket beyond each end, plain and (where the entry is a SwiGLU shape) paired
    for (mb, N, K, *_rest) in G.TUNED:
        for b in range(mb - 2, mb + 3):
            for M in (64 * b - 63, 64 * b):
                for act in (0, 4):
                    if M < 1 or (act == 4 and (K % 64 or N % 8)):
                        continue
                    c = dict(case, M=M, N=N, K=K, act=act)
                    want, got = G.plan_of(c), _host_plan(lib, c, None)
                    assert got == {k: want[k] for k in got}, (M, N, K, act, got, want)
                    n += 1
    print(f"{n} plans compared")


def test_case_list_covers_every_kernel_and_edge():
    ids = [c["id"] for c in G.CASES]
    assert len(set(ids)) == len(ids), "duplicate case ids"
    unforced, forced = {}, {}
    for c in G.CASES:
        p = G.plan_of(c)
        unforced.setdefault((p["kernel"], "split" if p["splits"] > 1 else "unsplit"), []).append(c)
        if c["force"]:
            pf = G.plan_of(c, True)
            forced.setdefault((pf["kernel"], "split" if pf["splits"] > 1 else "unsplit"), []).append(c)
    print("kernel        form      unforced  forced")
    for kern, forms in G.KERNELS.items():
        for form in ("unsplit", "split"):
            print(f"{kern:13s} {form:8s} {len(unforced.get((kern, form), [])):8d} {len(forced.get((kern, form), [])):7d}")
    # what the product dispatch reaches, derived: every tuned-table entry across its row bucket (the table is the only way to several
    # kernels) and a grid for the cost model and the large-M rules -- KERNELS must state exactly that, and the cases must reach it all
    reach = {}
    shapes = [(64 * b - d, N, K, act) for (mb, N, K, *_r) in G.TUNED for b in (mb - 1, mb, mb + 1) for d in (63, 17, 0)
              for act in ((0, 4) if K % 64 == 0 and N % 8 == 0 else (0,))]
    shapes += [(M, N, K, 0) for K in (72, 200, 192, 512, 1000, 1176, 1280, 1536, 2048, 2056, 3584, 4096, 8960)
               for M in (1, 64, 70, 130, 275, 290, 1000, 1024, 2048, 2050, 2100, 2305, 4096) for N in (132, 260, 392, 1284, 1540, 2052, 3204, 3460, 6200)]
    for (M, N, K, act) in shapes:
        if M >= 1:
            p = G.plan_bf16(M, N, K, act=act)
            reach.setdefault(p["kernel"], set()).add("split" if p["splits"] > 1 else "unsplit")
    for kern, forms in G.KERNELS.items():
        if not kern.startswith("fp8"):
            assert reach.get(kern, set()) == forms, f"KERNELS[{kern}] = {forms} but the sweep reaches {reach.get(kern, set())}"
    for kern, forms in G.KERNELS.items():
        for form in forms:
            assert unforced.get((kern, form)), f"no unforced case reaches {kern} {form}"
        assert not (set(f for (k, f) in unforced if k == kern) - forms), f"KERNELS understates what the product reaches for {kern}"
    splittable = lambda k: k not in ("glds<2,2>", "glds<4,2>", "glds<2,3,4>")
    for kern in G.KERNELS:
        if kern.startswith("fp8"):
            continue
        for form in ("unsplit", "split"):
            if form == "split" and not splittable(kern):
                continue
            cs = forced.get((kern, form), [])
            ragged = [c for c in cs if c["M"] % G.FORCE_BM[kern] and c["N"] % 128 == 4 and c["N"] > 128
                      and (form == "unsplit" or c["K"] % G.plan_of(c, True)["kps"])]           # split: with a K tail
            assert [c for c in ragged if not c["bias"] and not c["inplace"] and not c["act"]], f"{kern} {form}: no forced plain case"
            assert [c for c in ragged if c["bias"] and c["inplace"]], f"{kern} {form}: no forced bias + in-place residual case"
            if form == "split":
                assert {c["act"] for c in ragged} >= {1, 2, 3}, f"{kern}: not every activation goes through the forced split-K reduce"
    # tall tiles at their edges; the 320-row table bucket's ends unforced
    for bm in (128, 192, 256, 320):
        kern = {128: ("glds<4,3>", "glds<2,2>", "glds<4,2>"), 192: ("glds<6,3>",), 256: ("glds<4,3,4>",), 320: ("glds<10,2>",)}[bm]
        ms = {c["M"] for c in G.CASES if c["force"] and G.plan_of(c, True)["bm"] == bm}
        assert {bm - 1, bm, bm + 1} <= ms, (bm, sorted(ms))
    m320 = {c["M"] for c in G.CASES if not c["force"] and G.plan_of(c)["kernel"] == "glds<10,2>"}
    assert {193, 384, 319, 320, 321} <= m320, sorted(m320)
    m256 = {c["M"] % 256 for c in G.CASES if not c["force"] and G.plan_of(c)["kernel"] == "glds<4,3,4>"}
    assert {255, 0, 1} <= m256, sorted(m256)
    # leading dimensions: one split and one unsplit case per family, and the fused norm
    fam = lambda k: "reg" if k.startswith("reg") else {"glds<2,2>": "dma64", "glds<2,3>": "dma64", "glds<4,2>": "dma128", "glds<4,3>": "dma128",
                                                       "glds<2,3,4>": "dma128", "glds<4,3,4>": "256", "glds<10,2>": "320", "glds<6,3>": "192"}.get(k, k)
    ld = set()
    for c in G.CASES:
        if c["ld"]:
            p = G.plan_of(c, bool(c["force"]))
            ld.add((fam(p["kernel"]), p["splits"] > 1))
    for f in ("reg", "dma64", "dma128", "256", "320"):
        assert (f, True) in ld and (f, False) in ld, (f, sorted(ld))
    assert [c for c in G.CASES if c["ld"] and c["norm"] and c["kind"] == "bf16"]
    # fp8: forced splits 1..8 with a tail, the 128-row tile, the norm-forced split, normq, ragged shapes
    f8 = [c for c in G.CASES if c["kind"] == "fp8"]
    got = {int(c["force"]["SVLM_GEMM8_SPLITS"]) for c in f8 if c["force"] and "SVLM_GEMM8_SPLITS" in c["force"] and c["K"] % 512}
    assert got >= set(range(1, 9)), got
    assert [c for c in f8 if c["force"] and G.plan_of(c, True)["kernel"] == "fp8<4,3>"]
    assert [c for c in f8 if c["norm"] and G.plan_fp8(c["M"], c["N"], c["K"])["splits"] == 1 and G.plan_of(c)["splits"] == 2]
    assert [c for c in f8 if c["note"] == "normq"] and [c for c in f8 if c["M"] % 64 and c["N"] % 128]
    # the exact generator stays bf16-exact (|K / 128 terms of one sign| + bias 2 + residual 3) and has no period a K-split could hide
    # in: the constant along one output's k is non-zero for two (m, n) in three, so every split's slab carries weight
    for c in G.CASES:
        if c["gen"] == "exact":
            assert c["K"] // 128 + 1 + 2 + 3 <= 256
    o = G.operands("exact", 7, 132, 1152)
    part = o["A"].float() @ o["W"].float().t()                     # one 1152-k slab (3 x 384, the period of the plain (m + k) % 3 pattern)
    assert float((part != 0).float().mean()) > 0.6 and float(part.abs().max()) == 9.0


def test_no_test_sets_a_tuning_switch_the_product_library_cannot_see():
    """The product library reads no environment (svlm_env() returns nullptr without -DSVLM_TUNING), so a test that sets SVLM_* with
    monkeypatch / os.environ and then calls the product HipOps forces nothing.  Switches go through helpers.forced_switches (with
    helpers.diag_ops), which serves the diagnostic library, whose reported plan the caller asserts.  Caught: a literal SVLM_ name in a
    setenv / putenv / environ[...] / environ.update / .update( call on the same line, in any test module but helpers.py."""
    pat = re.compile(r"""(setenv\(\s*["']SVLM_|environ\[\s*["']SVLM_|putenv\(\s*["']SVLM_|(environ|update\(|setdefault\().*["']SVLM_)""")
    allowed = {"test_gemm_ref64.py", "helpers.py"}         # this file (the pattern above); the fixture itself
    bad = []
    for fn in sorted(os.listdir(os.path.join(ROOT, "tests"))):
        if fn.endswith(".py") and fn not in allowed:
            for i, line in enumerate(open(os.path.join(ROOT, "tests", fn)), 1):
                if pat.search(line) and "SVLM_LIB_PATH" not in line and "forced_switches(" not in line:
                    bad.append(f"tests/{fn}:{i}: {line.strip()}")
    assert not bad, "tuning switches set outside the diagnostic fixture:\n" + "\n".join(bad)
