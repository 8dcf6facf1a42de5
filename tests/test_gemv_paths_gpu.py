"""Every form of the decode GEMVs (csrc/gemv.hip, decode_fused.hip, decode_fp8.hip, decode_fp4.hip) on the MI355X, through the product
HipOps and the product dispatch, against the fp64 reference and the derived per-element bound of tests/gemv_ref64.py, over the case
list of tests/gemv_paths.py (whose ids name the form: family.kind.r<rows per wave>[k<KW>]p<PRE>[x<XC>]).

Every case checks the sentinels behind its output; `bits` probes are compared bit for bit; the fused kernels are compared with the
fp64 GEMV of their OWN staged activation row, recovered through an identity weight matrix (test_staged_row_*: that row against the
fp64 RMSNorm, and bitwise equal across the three families, which share dec_xrow.h:stage_x)."""
import zlib

import pytest
import torch

import gemv_paths as G
import gemv_ref64 as R

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
EPS = 1e-6
SENTINEL = 7.0


@pytest.fixture(scope="module")
def ops():
    from streaming_vlm_amd.ops import HipOps
    return HipOps()


# ------------------------------------------------------------------------------------------------ the staged row, through W = I
_IDENT = {}


def _identity(family, K):
    """Row slices [v0, v0 + V) of the K x K identity in the family's format (at most 4096 rows at a time): [(v0, V, tensors)]."""
    key = (family, K)
    if key not in _IDENT:
        _IDENT.clear()                                  # one K at a time: 4096 x 8192 bf16 is 64 MiB
        out = []
        for v0 in range(0, K, 4096):
            V = min(4096, K - v0)
            extra = 2 if family == "fp4" else 0         # dec_qkv_fp4: one key and one value row behind the V query rows, all zero
            hot = torch.zeros((V + extra, K), dtype=torch.uint8, device="cuda")
            hot[torch.arange(V), v0 + torch.arange(V)] = 1
            if family == "bf16":
                t = (hot.to(BF16),)
            elif family == "fp8":
                t = ((hot * 0x38).view(torch.float8_e4m3fn), torch.ones(V, device="cuda"))
            else:
                t = (G.e2m1_pack(hot * 2), torch.full((V + 2, K // 32), 127, dtype=torch.uint8, device="cuda"))
            out.append((v0, V, t))
        _IDENT[key] = out
    return _IDENT[key]


def staged_row(ops, family, x, gain):
    """xs of dec_xrow.h:stage_x as the kernels of `family` see it at this K: bf16 (K,) on the CPU, bit for bit."""
    K = x.numel()
    xs = torch.empty(K, dtype=torch.float32, device="cuda")
    xg, gg = x.cuda(), gain.cuda()
    for v0, V, t in _identity(family, K):
        if family == "fp4":
            pool = torch.zeros((1, 2, 1, 1, 1), dtype=BF16, device="cuda")
            q = torch.full((V,), SENTINEL, dtype=BF16, device="cuda")
            ops.dec_qkv_fp4(xg, gg, EPS, t[0], t[1], torch.zeros(V + 2, dtype=BF16, device="cuda"), q, pool, 0,
                            torch.zeros(1, dtype=torch.int32, device="cuda"), V, 1, length=0)
            assert float(pool.abs().max()) == 0.0
            xs[v0:v0 + V] = q.float()
            continue
        logits = torch.full((V,), SENTINEL, dtype=torch.float32, device="cuda")
        ws = torch.empty(ops.lib.svlm_dec_lm_head_ws_bytes(V) // 4 + 1, dtype=torch.float32, device="cuda")
        if family == "bf16":
            ops.dec_lm_head(xg, gg, EPS, t[0], logits, None, 1.0, None, ws)
        else:
            ops.dec_lm_head_fp8(xg, gg, EPS, t[0], t[1], logits, None, 1.0, None, ws)
        xs[v0:v0 + V] = logits
    xs = xs.cpu()
    assert torch.equal(xs.to(BF16).float(), xs), "the staged row must be bf16 values"
    return xs.to(BF16)


FUSED_KS = sorted({c["K"] for c in G.CASES if c["kind"] != "gemv"})


@pytest.mark.parametrize("K", FUSED_KS)
def test_staged_row_against_fp64_rmsnorm_and_equal_across_families(ops, K):
    """(a) xs against the fp64 RMSNorm of x under norm_reference's RMS bound, x at scale 2.5 and a gain over a decade, in every family
    that takes this K; the families' rows equal value for value (the fp4 row comes through `+ 0` of a zero bias, which loses the sign of a zero)."""
    x, gain = G.activation_row("iid", K, True)
    ref, bound = R.xs_reference(x, gain, EPS)
    rows = {}
    for family in G.FAMILIES:
        if K % G.VEC[family]:
            continue
        rows[family] = staged_row(ops, family, x, gain)
        R.check(f"xs {family} K={K}", rows[family].reshape(1, -1), ref.reshape(1, -1), bound.reshape(1, -1))
    assert rows
    first = next(iter(rows.values()))
    for family, xs in rows.items():
        assert torch.equal(xs.float(), first.float()), f"staged row of {family} differs from {next(iter(rows))} at K={K}"


# ------------------------------------------------------------------------------------------------ one launch per kind
def _w_args(case, o):
    family = case["family"]
    W = G.pad_rows(family, o) if case["pad"] else o[{"bf16": "W", "fp8": "W8", "fp4": "W4"}[family]]
    if case["pad"]:
        assert W.stride(0) > W.shape[1]
    return (W,) if family == "bf16" else (W, o["s8"]) if family == "fp8" else (W, o["s4"])


def _guard(n, dtype):
    return torch.full((n + 8,), SENTINEL, dtype=dtype, device="cuda")


def _untouched(guard, n, what):
    assert bool((guard[n:] == SENTINEL).all()), f"{what}: elements behind the output were written"


def launch(ops, case, wargs, x, gain, bias, res):
    """-> the N stored outputs (float32 on the CPU) of one launch of the case's entry point."""
    family, kind, N, K = case["family"], case["kind"], case["N"], case["K"]
    xg = x.cuda()
    if kind == "gemv":
        fn = {"bf16": ops.gemv, "fp8": ops.gemv_fp8, "fp4": ops.gemv_fp4}[family]
        gb, gf = _guard(N, BF16), _guard(N, torch.float32)
        kw = dict(bias=None if bias is None else bias.cuda(), residual=None if res is None else res.cuda(), out=gb[:N])
        if case["inplace"]:                              # out = residual = the hidden state, as the decode step calls it
            gb[:N] = res.cuda()
            kw["residual"] = gb[:N]
        if case["f32"]:
            kw["out_f32"] = gf[:N]
        if family == "bf16":
            kw["act"] = case["act"]
        fn(xg, *wargs, **kw)
        _untouched(gb, N, case["id"])
        _untouched(gf, N, case["id"])
        y = gb[:N].float().cpu()
        if case["f32"]:
            assert torch.equal(gf[:N].cpu(), y), "the fp32 output must be the bf16 output's value"
        return y
    gg = gain.cuda()
    if kind == "gate_up":
        fn = {"bf16": ops.dec_gate_up, "fp8": ops.dec_gate_up_fp8, "fp4": ops.dec_gate_up_fp4}[family]
        gh = _guard(N, BF16)
        fn(xg, gg, EPS, *wargs, gh[:N])
        _untouched(gh, N, case["id"])
        return gh[:N].float().cpu()
    if kind == "lm_head":
        gl = _guard(N, torch.float32)
        ws = torch.empty(ops.lib.svlm_dec_lm_head_ws_bytes(N) // 4 + 1, dtype=torch.float32, device="cuda")
        if family == "bf16":
            ops.dec_lm_head(xg, gg, EPS, *wargs, gl[:N], None, 1.0, None, ws)
        else:
            ops.dec_lm_head_fp8(xg, gg, EPS, *wargs, gl[:N], None, 1.0, None, ws)
        _untouched(gl, N, case["id"])
        y = gl[:N].cpu()
        assert torch.equal(y.to(BF16).float(), y), "logits must be bf16 values"
        return y
    q = case["qkv"]
    D, qd, kd = q["D"], q["Hq"] * q["D"], q["Hkv"] * q["D"]
    pool = (torch.randn((2, 2, q["Hkv"], 6, D), generator=torch.Generator().manual_seed(5)).to(BF16)).cuda()
    pool0 = pool.clone()
    slot_of = torch.tensor([3, 1, 4, 0, 5, 2], dtype=torch.int32, device="cuda")
    gq = _guard(qd, BF16)
    fn = {"bf16": ops.dec_qkv, "fp8": ops.dec_qkv_fp8, "fp4": ops.dec_qkv_fp4}[family]
    fn(xg, gg, EPS, *wargs, bias.cuda(), gq[:qd], pool, 1, slot_of, qd, kd, length=2)
    _untouched(gq, qd, case["id"])
    y = torch.cat([gq[:qd], pool[1, 0, :, 4, :].reshape(-1), pool[1, 1, :, 4, :].reshape(-1)]).float().cpu()
    pool[1, :, :, 4, :] = pool0[1, :, :, 4, :]
    assert torch.equal(pool, pool0), "dec_qkv wrote outside the new token's slot"
    return y


@pytest.mark.parametrize("case", G.CASES, ids=[c["id"] for c in G.CASES])
def test_gemv_form_against_fp64_bound(ops, case):
    family, kind, N, K, f = case["family"], case["kind"], case["N"], case["K"], case["form"]
    assert G.form_key(G.form(family, kind, N, K)) == G.form_key(f)
    fused = kind != "gemv"
    seed = zlib.crc32(case["id"].encode()) % 1000
    for gen in case["gens"]:
        o = G.weights(family, gen, 2 * N if kind == "gate_up" else N, K, seed=seed, device="cuda")
        bias, res = G.epilogue_operands(gen, N, K, o["row_exp"][:N], case["bias"], case["res"], seed=seed)
        c = R.fadds(f, bias is not None)
        wargs = _w_args(case, o)
        x0, gain = G.activation_row(gen, K, fused, seed=seed)
        # N = 1: one output says nothing about a mean, so 32 activation rows are run and their outputs checked as one vector
        probes = G.bits_probes(K) if gen == "bits" else [x0] if N > 1 else [G.activation_row(gen, K, fused, seed=seed + j)[0] for j in range(32)]
        if gen == "bits" and fused:
            gain = torch.ones(K, dtype=BF16)
        worst = mean = 0.0
        pooled = []
        for i, x in enumerate(probes):
            xd = x
            if fused:
                xd = staged_row(ops, family, x, gain)
                if gen == "bits":
                    assert torch.equal(xd.float(), x.float()), f"{case['id']} probe {i}: gain 1 and x = +-1 must stage x itself"
            got = launch(ops, case, wargs, x, gain, bias, res)
            if gen == "bits":
                ref, bound = R.bits_reference(kind, o["Wf"], xd, bias, res)
            else:
                ref, bound = R.reference(kind, o["Wf"], xd, c, bias, res, case["act"])
            if N == 1:
                pooled.append((got, ref, bound))
                continue
            w, m = R.check_rows(f"{case['id']} {gen} probe {i}", got, ref, bound, f)
            worst, mean = max(worst, w), max(mean, m)
        if pooled:
            worst, mean = R.check_rows(f"{case['id']} {gen} row 0 of {len(pooled)} activation rows (listed as rows)",
                                       *(torch.cat(t) for t in zip(*pooled)), f)
        print(f"[gemv-path] {f['name']} {gen} N={N} K={K} c={c}: worst err/bound {worst:.3f} mean {mean:.3f}")
