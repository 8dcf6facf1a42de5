"""CPU checks of the decode GEMV path test machinery (no GPU): the fp64 reference and bound of tests/gemv_ref64.py against the bf16 CPU
oracle, against an fp32 emulation of every kernel form in the kernel's lane and chain order, and against injected faults; the coverage
conditions of the case list of tests/gemv_paths.py; and a pin of the dispatch literals the mirror restates on the launchers' source."""
import os

import pytest
import torch

import gemv_paths as G
import gemv_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "streaming-vlm_amd", "csrc")
BF16 = torch.bfloat16
EPS = 1e-6


def _ops(family, gen, kind, N, K, bias=True, res=True, seed=0):
    o = G.weights(family, gen, 2 * N if kind == "gate_up" else N, K, seed=seed)
    o["bias"], o["res"] = G.epilogue_operands(gen, N, K, o["row_exp"][:N], bias, res, seed=seed)
    o["x"], o["gain"] = G.activation_row(gen, K, kind != "gemv", seed=seed)
    return o


def _codes(family, o):
    """What emulate() multiplies: the fp8 codes as float and the row scales, W' itself elsewhere."""
    return (o["W8"].float(), o["s8"]) if family == "fp8" else (o["Wf"], None)


# ------------------------------------------------------------------------------------------------ the CPU oracle
@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("gen,N,K", [("iid", 133, 1056), ("spread", 70, 4128), ("spread", 133, 96)])
def test_cpu_oracle_is_within_the_bound(family, gen, N, K):
    """RefOps (F.linear in bf16, fp32 accumulation inside) on the dequantised weights makes the kernels' roundings; c = K + 1: one fp32
    addition per product at the very most (a sequential sum) and the bias.  The fused ops against the oracle's own normalised row."""
    from oracle import model as om
    from ref_ops import RefOps
    ref_ops = RefOps()
    o = _ops(family, gen, "gemv", N, K)
    W = o["Wf"].to(BF16)
    assert torch.equal(W.float(), o["Wf"]), "W' is exact in bf16"
    for bias, res in ((o["bias"], None), (None, o["res"]), (o["bias"], o["res"])):
        y = ref_ops.gemv(o["x"], W, bias=bias, residual=res, out=torch.empty(N, dtype=BF16))
        R.check_rows(f"oracle gemv {family} {gen}", y, *R.reference("gemv", o["Wf"], o["x"], K + 1, bias, res), G.form(family, "gemv", N, K))
    x, gain = G.activation_row(gen, K, True)
    xs = om.rms_norm(x.reshape(1, -1), gain, EPS)[0]
    R.check("oracle xs", xs.reshape(1, -1), *[t.reshape(1, -1) for t in R.xs_reference(x, gain, EPS)])
    D, qd = 20, N - 2 * 20                       # dec_qkv: head_dim 20, one key/value head
    pool = torch.zeros((1, 2, 1, 2, D), dtype=BF16)
    q = torch.zeros(qd, dtype=BF16)
    ref_ops.dec_qkv(x, gain, EPS, W, o["bias"], q, pool, 0, torch.tensor([1, 0], dtype=torch.int32), qd, D, length=0)
    y = torch.cat([q, pool[0, 0, 0, 1], pool[0, 1, 0, 1]])
    R.check_rows("oracle dec_qkv", y, *R.reference("qkv", o["Wf"], xs, K + 1, o["bias"]), G.form(family, "qkv", N, K))
    logits = torch.zeros(N)
    ref_ops.dec_lm_head(x, gain, EPS, W, logits, None, 1.0, None, None)
    R.check_rows("oracle dec_lm_head", logits, *R.reference("lm_head", o["Wf"], xs, K), G.form("bf16", "lm_head", N, K))
    g = _ops(family, gen, "gate_up", N, K, seed=1)
    h = torch.zeros(N, dtype=BF16)
    ref_ops.dec_gate_up(x, gain, EPS, g["Wf"].to(BF16), h)
    R.check_rows("oracle dec_gate_up", h, *R.reference("gate_up", g["Wf"], xs, K), G.form(family, "gate_up", N, K))


# ------------------------------------------------------------------------------------------------ the emulation of every form
def _form_shapes():
    """One (family, kind, N of the form, ragged K) per form the product reaches, plus a second ragged K for the K-split forms."""
    out, seen = [], set()
    for c in G.CASES:
        key = G.form_key(c["form"])
        if key in seen or c["K"] < 64:
            continue
        seen.add(key)
        out.append((c["family"], c["kind"], c["N"], c["K"]))
    return out


@pytest.mark.parametrize("family,kind,N,K", _form_shapes(), ids=lambda v: str(v))
def test_emulation_of_each_form_is_within_the_bound(family, kind, N, K):
    """fp32 in the kernel's lane, chain, butterfly and partial order (6 rows of the form's matrix are enough: rows do not interact), with
    spread operands: inside the bound with the form's own c."""
    f = G.form(family, kind, N, K)
    rows = 6
    o = _ops(family, "spread", kind, rows, K, bias=kind in ("gemv", "qkv"), res=kind == "gemv", seed=K % 97)
    Wq, scale = _codes(family, o)
    c = R.fadds(f, o["bias"] is not None)
    x = o["x"]
    if kind != "gemv":
        from oracle import model as om
        x = om.rms_norm(o["x"].reshape(1, -1), o["gain"], EPS)[0]
    got = R.emulate(f, Wq, x, scale, o["bias"], o["res"])
    worst, mean = R.check_rows(f"emulated {f['name']} K={K}", got, *R.reference(kind, o["Wf"], x, c, o["bias"], o["res"]), f)
    assert worst > 0.0


def test_emulation_with_each_activation():
    f = G.form("bf16", "gemv", 133, 1032)
    o = _ops("bf16", "spread", "gemv", 133, 1032)
    for act in (1, 2, 3):
        got = R.emulate(f, o["Wf"], o["x"], None, o["bias"], o["res"], act=act)
        R.check_rows(f"emulated act {act}", got, *R.reference("gemv", o["Wf"], o["x"], R.fadds(f, True), o["bias"], o["res"], act), f)


# ------------------------------------------------------------------------------------------------ injected faults
SPLIT_K = {"bf16": 4104, "fp8": 4112, "fp4": 4128}


def _faults(family, o, f, Wq, scale, bound=None):
    """-> [(name, emulated faulty output, |change of the Linear output| per row in fp64)]."""
    K, vec = Wq.shape[1], f["vec"]
    N = Wq.shape[0]
    x, b, r = o["x"], o["bias"], o["res"]
    out = []
    c0 = f["ranges"][-1][0] + vec * 3                       # a vector of the last wave's range (the short one)
    for name, factor in (("vector zeroed", 0.0), ("vector doubled", 2.0)):
        x2 = x.clone()
        x2[c0:c0 + vec] = (x2[c0:c0 + vec].float() * factor).to(BF16)
        out.append((name, R.emulate(f, Wq, x2, scale, b, r), (o["Wf"].double() @ (x2.double() - x.double())).abs()))
    if f["kw"] > 1:                                         # wave 1 drops its first vector and takes wave 2's first one again
        lo, hi = f["ranges"][1]
        d = o["Wf"][:, hi:hi + vec].double() @ x[hi:hi + vec].double() - o["Wf"][:, lo:lo + vec].double() @ x[lo:lo + vec].double()
        out.append(("split range shifted", R.emulate(f, Wq, x, scale, b, r, shift_wave=(1, 1)), d.abs()))
    def worst_row(change):                                  # the row where the fault is most visible (bits: any row will do)
        return 5 if bound is None else int((change / bound[:N - 1]).argmax())

    def one(n, v):
        d = torch.zeros(N, dtype=torch.float64)
        d[n] = v
        return d
    db, dr = (b[1:].double() - b[:-1].double()).abs(), (r[1:].double() - r[:-1].double()).abs()
    n = worst_row(db)
    b2 = b.clone()
    b2[n] = b[n + 1]
    out.append(("neighbour's bias", R.emulate(f, Wq, x, scale, b2, r), one(n, db[n])))
    n = worst_row(dr)
    r2 = r.clone()
    r2[n] = r[n + 1]
    out.append(("neighbour's residual", R.emulate(f, Wq, x, scale, b, r2), one(n, dr[n])))
    if family == "fp8":
        ds = ((Wq.double() @ x.double())[:-1] * (scale[1:].double() - scale[:-1].double())).abs()
        n = worst_row(ds)
        s2 = scale.clone()
        s2[n] = scale[n + 1]
        out.append(("neighbour's scale", R.emulate(f, Wq, x, s2, b, r), one(n, ds[n])))
    if family == "fp4":
        from streaming_vlm_amd.weights import dequantize_blocks_mxfp4
        nb = K // 32
        contrib = (o["Wf"].double() * x.double()[None, :]).view(N, nb, 32).sum(dim=2)[:, :-1]              # per (row, block)
        e = o["s4"].to(torch.int32)
        dblk = (contrib * (torch.pow(2.0, (e[:, 1:] - e[:, :-1]).double()) - 1)).abs()
        flat = int((dblk if bound is None else dblk / bound[:, None]).argmax())
        n, blk = flat // (nb - 1), flat % (nb - 1)
        s2 = o["s4"].clone()
        s2[n, blk] = o["s4"][n, blk + 1]
        W2 = dequantize_blocks_mxfp4(o["W4"], s2, torch.float32)
        out.append(("neighbour block's scale", R.emulate(f, W2, x, None, b, r), ((W2.double() - o["Wf"].double()) @ x.double()).abs()))
    return out


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("split", [False, True])
def test_injected_faults_fail_exactly_under_bits(family, split):
    """Every fault changes an exact sum of the bits output for some probe, so bit equality fails (the all-ones probe sees a dropped or
    doubled column, a bit probe a weight paired with another column's x)."""
    N, K = 133, SPLIT_K[family] if split else 1024 + G.VEC[family]
    f = G.form(family, "gemv", N, K)
    assert (f["kw"] > 1) == split
    o = _ops(family, "bits", "gemv", N, K)
    Wq, scale = _codes(family, o)
    caught = {}
    for i, x in enumerate(G.bits_probes(K)):
        o["x"] = x
        ref, bound = R.bits_reference("gemv", o["Wf"], x, o["bias"], o["res"])
        assert bound is None
        R.check_rows(f"bits clean probe {i}", R.emulate(f, Wq, x, scale, o["bias"], o["res"]), ref, None, f)
        for name, bad, _ in _faults(family, o, f, Wq, scale):
            try:
                R.check_rows(f"bits {name} probe {i}", bad, ref, None, f)
                caught.setdefault(name, False)
            except AssertionError as e:
                assert "differ" in str(e) and f["name"] in str(e)
                caught[name] = True
    assert caught and all(caught.values()), caught


@pytest.mark.parametrize("family", G.FAMILIES)
@pytest.mark.parametrize("gen", ["iid", "spread"])
@pytest.mark.parametrize("split", [False, True])
def test_injected_faults_fail_the_bound_wherever_a_product_is_visible(family, gen, split):
    """iid / spread: a fault MUST fail in every row where it moves the Linear output by more than twice the row's bound (the clean
    kernel is within one bound of the reference, so the faulty one is more than one bound away); computed here, not assumed, and every
    fault has such a row at these shapes."""
    N, K = 133, SPLIT_K[family] if split else 1024 + G.VEC[family]
    f = G.form(family, "gemv", N, K)
    o = _ops(family, gen, "gemv", N, K)
    Wq, scale = _codes(family, o)
    ref, bound = R.reference("gemv", o["Wf"], o["x"], R.fadds(f, True), o["bias"], o["res"])
    R.check_rows("clean", R.emulate(f, Wq, o["x"], scale, o["bias"], o["res"]), ref, bound, f)
    for name, bad, delta in _faults(family, o, f, Wq, scale, bound):
        must = delta > 2 * bound
        if name == "neighbour's scale" and gen == "iid" and not bool(must.any()):
            continue                                        # iid rows can all share one power-of-two scale: then there is no such fault
        assert bool(must.any()), f"{name}: pick a shape where the fault is visible"
        ratio, _ = R.ratios(bad, ref, bound)
        assert bool((ratio[must] > 1).all()), name
        with pytest.raises(AssertionError, match="rows off"):
            R.check_rows(name, bad, ref, bound, f)
    # a systematic error of 0.65 roundings on every element stays under the per-element bound and fails the mean
    with pytest.raises(AssertionError, match="mean err/bound"):
        R.check_rows("systematic", ref + 0.65 * bound, ref, bound, f)


def test_a_removed_rounding_and_a_stale_staged_element_fail_under_bits():
    """fp4 bits: the blocks of a row carry different scales, so an exact sum is generally NOT a bf16 value and the rounding of the Linear
    output in front of the residual add is visible bit for bit (asserted on the data).  A reference in fp64 cannot see a MISSING
    rounding under iid operands -- the output only gets closer to it -- which is what the bits operands are for.  A stale element of the
    staged row (xs[j] of the previous token) changes every row with a one in column j."""
    N, K = 133, 2080
    f = G.form("fp4", "gemv", N, K)
    o = _ops("fp4", "bits", "gemv", N, K)
    x = G.bits_probes(K)[3]
    ref, _ = R.bits_reference("gemv", o["Wf"], x, o["bias"], o["res"])
    z = R.dot64(o["Wf"], x)[0] + o["bias"].double()
    assert bool((z.float().to(BF16).double() != z).any()), "bits fp4: some exact sums must not be bf16 values"
    R.check_rows("clean", R.emulate(f, o["Wf"], x, None, o["bias"], o["res"]), ref, None, f)
    with pytest.raises(AssertionError, match="differ"):
        R.check_rows("rbf removed", R.emulate(f, o["Wf"], x, None, o["bias"], o["res"], drop_rbf=True), ref, None, f)
    g = G.form("fp4", "gate_up", N, K)
    w = _ops("fp4", "bits", "gate_up", N, K)
    refg, boundg = R.bits_reference("gate_up", w["Wf"], x)
    R.check_rows("gate_up clean", R.emulate(g, w["Wf"], x), refg, boundg, g)
    stale = x.clone()
    stale[77] = -stale[77]
    with pytest.raises(AssertionError, match="rows off"):
        R.check_rows("stale xs", R.emulate(g, w["Wf"], stale), refg, boundg, g)
    ql = G.form("fp4", "qkv", N, K)
    refq, _ = R.bits_reference("qkv", o["Wf"], x, o["bias"])
    with pytest.raises(AssertionError, match="differ"):
        R.check_rows("stale xs qkv", R.emulate(ql, o["Wf"], stale, None, o["bias"]), refq, None, ql)


# ------------------------------------------------------------------------------------------------ the case list and the mirror
def test_case_list_meets_the_coverage_conditions():
    ids = [c["id"] for c in G.CASES]
    assert len(ids) == len(set(ids)) and len(ids) <= 160
    reach = G.reachable()
    by_form = {}
    for c in G.CASES:
        assert G.form_key(G.form(c["family"], c["kind"], c["N"], c["K"])) == G.form_key(c["form"])
        by_form.setdefault(G.form_key(c["form"]), []).append(c)
    assert set(by_form) == set(reach), set(reach) ^ set(by_form)
    assert len(reach) == 43
    for key, info in reach.items():
        cs = by_form[key]
        have = set().union(*(G.k_conditions(c["form"], c["K"]) for c in cs))
        assert info["conds"] <= have, (info["name"], info["conds"] - have)          # every ragged-K condition the form admits
        assert any("bits" in c["gens"] for c in cs), info["name"]
        assert any("iid" in c["gens"] for c in cs) and any("spread" in c["gens"] for c in cs), info["name"]
        assert any(c["N"] % c["form"]["wg_rows"] for c in cs), info["name"]          # a last workgroup with clamped rows
    for family in G.FAMILIES:
        fam = [c for c in G.CASES if c["family"] == family]
        gv = [c for c in fam if c["kind"] == "gemv"]
        for split in (False, True):
            sp = [c for c in gv if (c["form"]["kw"] > 1) == split]
            assert any(c["N"] == 1 for c in sp)
            assert any(c["bias"] and not c["res"] for c in sp) and any(c["bias"] and c["res"] for c in sp)
            assert any(c["f32"] for c in sp) and any(c["inplace"] for c in sp) and any(c["pad"] for c in sp)
        assert any(c["res"] and not c["bias"] for c in gv)
        assert any(c["form"]["rows"] == 2 and c["form"]["kw"] == 1 and c["pad"] for c in gv)
        for kind in G.KINDS[family][1:]:
            ks = [c for c in fam if c["kind"] == kind]
            assert any(c["pad"] for c in ks)
            assert kind == "qkv" or any(c["N"] == 1 for c in ks)
        qk = [c for c in fam if c["kind"] == "qkv"]
        assert any(c["qkv"]["D"] != 128 and c["N"] % 4 for c in qk) and any(c["qkv"]["D"] == 128 for c in qk)
        for (N, K) in ((1536, 1536), (1536, 8960), (3584, 3584), (3584, 18944)):
            assert any(c["N"] == N and c["K"] == K and {"iid", "spread"} <= set(c["gens"]) for c in gv), (family, N, K)
        assert all(c["K"] <= 8192 for c in fam if c["kind"] != "gemv") and all(c["N"] <= 5000 for c in fam if c["kind"] == "lm_head")
    assert {c["act"] for c in G.CASES if c["family"] == "bf16" and c["kind"] == "gemv"} == {0, 1, 2, 3}
    # the examples the kernels' arithmetic gives: per-wave share kq and the batch it overruns by one vector
    for family, K, kq in (("bf16", 4104, 1032), ("bf16", 10248, 2568), ("fp8", 4112, 1040), ("fp8", 12304, 3088), ("fp4", 4128, 1056),
                          ("fp4", 16416, 4128)):
        f = G.form(family, "gemv", 133, K)
        assert f["kw"] == 4 and f["ranges"][0] == (0, kq) and any(c["K"] == K and c["N"] == 133 for c in G.CASES if c["family"] == family)
    assert G.form("bf16", "gemv", 133, 4104)["ranges"][3] == (3096, 4104)          # the last wave: 1008
    assert G.form("bf16", "gemv", 16387, 1544)["pre"] == 3 and G.form("bf16", "gemv", 16387, 1544)["batch"] == 1536


PINS = {
    "gemv.hip": ["if (N <= 8192 && K >= 4096) {", "(force_rows == 0 && N >= 16384)", "(N >= 4096 || (long long)N * K >= (8LL << 20))",
                 "constexpr int PRE = ROWS >= 4 ? 3 : 4;", "constexpr int PRE = 5;", "#define KS_ROWS 2", "gemv_bf16_kernel<4><<<(N + 15) / 16",
                 "gemv_bf16_kernel<2><<<(N + 7) / 8", "gemv_bf16_kernel<1><<<(N + 3) / 4", "const int kq = ((K / 8 + 3) / 4) * 8;"],
    "decode_fused.hip": ["if ((K) <= 1536) KERNEL<ROWS, 3, 1> __VA_ARGS__;", "else if ((K) <= 2048) KERNEL<ROWS, 4, 1> __VA_ARGS__;",
                         "else if ((K) <= 4096) KERNEL<ROWS, 4, 2> __VA_ARGS__;", "else KERNEL<ROWS, 4, 4> __VA_ARGS__;", "#define GU_ROWS 1",
                         "#define LM_ROWS 2", "DEC_DISPATCH(dec_qkv_kernel, 1, K,", "K % 8 == 0 && K <= 8192"],
    "decode_fp8.hip": ["if ((K) <= 1024) KERNEL<ROWS, 1, 1> __VA_ARGS__;", "else if ((K) <= 2048) KERNEL<ROWS, 2, 1> __VA_ARGS__;",
                       "else if ((K) <= 4096) KERNEL<ROWS, 4, 2> __VA_ARGS__;", "else KERNEL<ROWS, 4, 4> __VA_ARGS__;", "#define QKV8_ROWS 1",
                       "#define GU8_ROWS 1", "#define LM8_ROWS 2", "if (N <= 8192 && K >= 4096) {", "gemv_fp8_kernel<2, 4, 3><<<(N + 1) / 2",
                       "} else if (N >= 16384) {", "gemv_fp8_kernel<4, 1, 2><<<(N + 15) / 16",
                       "} else if (N >= 4096 || (long long)N * K >= (8LL << 20)) {", "gemv_fp8_kernel<2, 1, 2><<<(N + 7) / 8",
                       "gemv_fp8_kernel<1, 1, 4><<<(N + 3) / 4", "const int kq = ((K / 16 + KW - 1) / KW) * 16;", "K % 16 == 0 && K <= 8192"],
    "decode_fp4.hip": ["if ((K) <= 2048) KERNEL<ROWS, 1, 1> __VA_ARGS__;", "else if ((K) <= 4096) KERNEL<ROWS, 2, 2> __VA_ARGS__;",
                       "else KERNEL<ROWS, 2, 4> __VA_ARGS__;", "#define QKV4_ROWS 1", "#define GU4_ROWS 1", "if (N <= 8192 && K >= 4096) {",
                       "gemv_fp4_kernel<2, 4, 2><<<(N + 1) / 2", "} else if (N >= 4096 || (long long)N * K >= (8LL << 20)) {",
                       "if (K <= 2048) gemv_fp4_kernel<2, 1, 1><<<(N + 7) / 8", "else gemv_fp4_kernel<2, 1, 2><<<(N + 7) / 8",
                       "if (K <= 2048) gemv_fp4_kernel<1, 1, 1><<<(N + 3) / 4", "else gemv_fp4_kernel<1, 1, 2><<<(N + 3) / 4",
                       "const int kq = ((K / 32 + KW - 1) / KW) * 32;", "K <= 8192"],
}


@pytest.mark.parametrize("name", sorted(PINS))
def test_dispatch_literals_the_mirror_restates_are_in_the_launchers(name):
    """gemv_paths.form() restates these lines; an edit of one of them has to come with an edit of the mirror (and of this pin)."""
    src = open(os.path.join(CSRC, name)).read()
    for lit in PINS[name]:
        assert src.count(lit) >= 1, f"{name}: `{lit}` is gone -- the dispatch changed; update tests/gemv_paths.py:form() and this pin"
    assert "N >= 16384" not in open(os.path.join(CSRC, "decode_fp4.hip")).read(), "fp4 has no 4-row form in the mirror"
