"""Python mirror of the decode GEMV dispatch (svlm_gemv_bf16 in csrc/gemv.hip, DEC_DISPATCH in csrc/decode_fused.hip, svlm_gemv_fp8 /
DEC8_DISPATCH in csrc/decode_fp8.hip, svlm_gemv_fp4 / DEC4_DISPATCH in csrc/decode_fp4.hip), the operand generators and the case list of
tests/test_gemv_paths_gpu.py (test helper, not product; needs no GPU).

A FORM is what one launch runs: (family, kind, rows per wave, KW waves sharing a row's K, PRE K-steps pre-issued per batch, XC chunks of
the staged activation row).  form() restates the launchers' conditions; tests/test_gemv_ref64.py pins the literals it restates against
the launchers' source, so a dispatch edit that is not mirrored here fails without a GPU.  Every form is reached through the product
dispatch by its shape alone (no tuning switch).

dec_qkv: N = qd + 2 kd with kd = Hkv * D; the wrapper admits any head_dim D without the linear planes (they need D = 128), so the ragged
qkv cases use D = 37 (qd = 111, kd = 37, N = 185 = 46 workgroups + 1 row).  N = 1 does not exist for it (N >= 3); the K-split form
and the one-row GEMVs, gate_up and lm_head have N = 1 cases."""
from __future__ import annotations

import math

import torch

BF16 = torch.bfloat16
FAMILIES = ("bf16", "fp8", "fp4")
VEC = {"bf16": 8, "fp8": 16, "fp4": 32}            # K elements of one 16-B weight load
STEP = {f: 64 * v for f, v in VEC.items()}         # K elements of one K-step of a wave
KINDS = {"bf16": ("gemv", "qkv", "gate_up", "lm_head"), "fp8": ("gemv", "qkv", "gate_up", "lm_head"), "fp4": ("gemv", "qkv", "gate_up")}
FUSED_MAX_K = 8192
ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF, ACT_SILU = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------ the mirror
def _fused_pre_xc(family, K):
    if family == "bf16":                               # DEC_DISPATCH
        return (3, 1) if K <= 1536 else (4, 1) if K <= 2048 else (4, 2) if K <= 4096 else (4, 4)
    if family == "fp8":                                # DEC8_DISPATCH
        return (1, 1) if K <= 1024 else (2, 1) if K <= 2048 else (4, 2) if K <= 4096 else (4, 4)
    return (1, 1) if K <= 2048 else (2, 2) if K <= 4096 else (2, 4)      # DEC4_DISPATCH


def form(family, kind, N, K):
    """-> dict(family, kind, rows, kw, pre, xc, vec, step, batch, wg_rows, dots, ranges, name).  N = output rows (gate_up: I).
    rows: output rows per wave; dots: weight rows a wave streams (gate_up: gate + up); wg_rows: output rows per workgroup;
    ranges: the (k_lo, k_hi) of the kw waves that share a row."""
    assert kind in KINDS[family], (family, kind)
    vec, step = VEC[family], STEP[family]
    assert N > 0 and K > 0 and K % vec == 0, (family, kind, N, K)
    xc = 0
    if kind == "gemv":
        if N <= 8192 and K >= 4096:                    # skinny output, long reduction: K split over the workgroup's 4 waves
            rows, kw, pre = 2, 4, {"bf16": 5, "fp8": 3, "fp4": 2}[family]
        elif family != "fp4" and N >= 16384:
            rows, kw, pre = 4, 1, {"bf16": 3, "fp8": 2}[family]
        elif N >= 4096 or N * K >= (8 << 20):
            rows, kw, pre = 2, 1, {"bf16": 4, "fp8": 2, "fp4": 1 if K <= 2048 else 2}[family]
        else:
            rows, kw, pre = 1, 1, {"bf16": 4, "fp8": 4, "fp4": 1 if K <= 2048 else 2}[family]
    else:
        assert K <= FUSED_MAX_K, (kind, K)
        rows, kw = (2 if kind == "lm_head" else 1), 1
        pre, xc = _fused_pre_xc(family, K)
    kq = ((K // vec + kw - 1) // kw) * vec
    ranges = [(p * kq, min(K, p * kq + kq)) for p in range(kw)]
    f = dict(family=family, kind=kind, rows=rows, kw=kw, pre=pre, xc=xc, vec=vec, step=step, batch=pre * step,
             wg_rows=rows * 4 // kw, dots=rows * (2 if kind == "gate_up" else 1), ranges=ranges)
    f["name"] = f"{family}.{kind}.r{rows}" + (f"k{kw}" if kw > 1 else "") + f"p{pre}" + (f"x{xc}" if xc else "")
    return f


def form_key(f):
    return (f["family"], f["kind"], f["rows"], f["kw"], f["pre"], f["xc"])


def lane_steps(f):
    """K-steps one lane executes (masked ones included: a whole batch is issued whenever one of its elements is in range)."""
    span = max(hi - lo for lo, hi in f["ranges"])
    return f["pre"] * max(1, -(-span // f["batch"]))


def k_conditions(f, K):
    """The ragged-edge conditions of the case list that hold for this form at this K."""
    out = set()
    if f["kw"] == 1:
        if K == f["vec"]:
            out.add("single_vector")
        if K % f["batch"] == 0:
            out.add("whole_batches")
        if K > f["batch"] and K % f["batch"] == f["vec"]:
            out.add("vector_past_batch")
    else:
        if (K // f["vec"]) % f["kw"]:
            out.add("short_last_wave")
        lo, hi = f["ranges"][0]
        if (hi - lo) > f["batch"] and (hi - lo) % f["batch"] == f["vec"]:
            out.add("vector_in_second_batch")
        if (hi - lo) % f["batch"] == 0:
            out.add("whole_batches")
    return out


# every (N, K) the reachability scan looks at: the N that select each row count, every K up to past the longest model row
SCAN_N = (1, 133, 2731, 4099, 8195, 16387)


def reachable():
    """-> {form key: {condition: True}} over the scan grid: which forms the product dispatch reaches and which K conditions each admits."""
    out = {}
    for family in FAMILIES:
        vec = VEC[family]
        for kind in KINDS[family]:
            for N in (SCAN_N if kind == "gemv" else (133,)):
                kmax = 19008 if kind == "gemv" else FUSED_MAX_K
                for K in range(vec, kmax + 1, vec):
                    f = form(family, kind, N, K)
                    d = out.setdefault(form_key(f), {"name": f["name"], "conds": set()})
                    d["conds"] |= k_conditions(f, K)
    return out


# ------------------------------------------------------------------------------------------------ operands
def _gen(seed, device="cpu"):
    return torch.Generator(device=device).manual_seed(seed)


def _pow2(e):
    return torch.pow(2.0, e.double()).float()


def e2m1_pack(code):
    """(N, K) nibbles -> (N, K / 2) bytes, element 2i in the low nibble of byte i."""
    return (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()


def bits_exponents(family, N, K, device="cpu"):
    """Power-of-two exponents of the `bits` weights: per row (bf16, fp8), per row and block (fp4); neighbours always differ."""
    n = torch.arange(N, device=device).view(N, 1)
    if family == "fp4":
        return ((3 * n + 5 * torch.arange(K // 32, device=device).view(1, -1)) % 9 - 4).to(torch.int32)          # (N, K / 32)
    return (n % 7 - 3).to(torch.int32)                                                             # (N, 1)


def bits_probes(K):
    """1 + ceil(log2 K) activation rows: all ones, then per bit b of the column index +1 where the bit is set and -1 elsewhere."""
    k = torch.arange(K)
    rows = [torch.ones(K)]
    for b in range(max(1, math.ceil(math.log2(K)))):
        rows.append(((k >> b) & 1).float() * 2 - 1)
    return [r.to(BF16) for r in rows]


def weights(family, gen, N, K, seed=0, device="cpu"):
    """-> dict(Wf float32 (N, K) = W' exactly; plus what the kernel reads: W (bf16) | W8, s8 | W4, s4), on `device`.
    iid: N(0, 0.05^2).  spread: rows (fp4: and blocks) scaled by 2^-6..2^6.  bits: W[n, k] = 2^e where k % 128 == n % 128, else 0."""
    from streaming_vlm_amd import weights as PW
    o = {"row_exp": torch.zeros(N, dtype=torch.int32, device=device)}
    if gen == "bits":
        assert N >= 128, "bits: every column must feed a row"
        e = bits_exponents(family, N, K, device)
        hot = (torch.arange(K, device=device).view(1, K) % 128) == (torch.arange(N, device=device).view(N, 1) % 128)
        if family == "bf16":
            o["Wf"] = hot.float() * _pow2(e)
            o["W"] = o["Wf"].to(BF16)
        elif family == "fp8":
            o["W8"] = (hot.to(torch.uint8) * 0x38).view(torch.float8_e4m3fn)
            o["s8"] = _pow2(e).view(N).contiguous()
            o["Wf"] = o["W8"].float() * o["s8"][:, None]
        else:
            o["W4"] = e2m1_pack(hot.to(torch.uint8) * 2)
            o["s4"] = (e + 127).to(torch.uint8).contiguous()
            o["Wf"] = PW.dequantize_blocks_mxfp4(o["W4"], o["s4"], torch.float32)
        assert torch.equal(o["Wf"] != 0, hot)
        return o
    g = _gen(1000 + seed, device)
    w = torch.randn((N, K), generator=g, device=device) * 0.05
    if gen == "spread":
        o["row_exp"] = torch.randint(-6, 7, (N,), generator=g, dtype=torch.int32, device=device)
        w = w * _pow2(o["row_exp"])[:, None]
        if family == "fp4":
            be = torch.randint(-6, 7, (N, K // 32), generator=g, dtype=torch.int32, device=device)
            w = (w.view(N, K // 32, 32) * _pow2(be)[:, :, None]).view(N, K)
    else:
        assert gen == "iid", gen
    w = w.to(BF16)
    if family == "bf16":
        o["W"], o["Wf"] = w, w.float()
    elif family == "fp8":
        o["W8"], o["s8"] = PW.quantize_rows_fp8_pow2(w)
        o["Wf"] = o["W8"].float() * o["s8"][:, None]
    else:
        o["W4"], o["s4"] = PW.quantize_blocks_mxfp4(w)
        o["Wf"] = PW.dequantize_blocks_mxfp4(o["W4"], o["s4"], torch.float32)
    return o


def epilogue_operands(gen, N, K, row_exp, bias, res, seed=0):
    """bias / residual (bf16, (N,)) or None.  bits: small integers.  iid / spread: at the scale of the row's output (0.05 sqrt(K)
    2^row_exp for unit-variance x), so that small outputs sit next to large ones."""
    n = torch.arange(N)
    if gen == "bits":
        return ((n % 5 - 2).to(BF16) if bias else None), ((n * 3 % 7 - 3).to(BF16) if res else None)
    g = _gen(2000 + seed)
    mag = 0.05 * math.sqrt(K) * _pow2(row_exp.cpu())
    b = (torch.randn(N, generator=g) * 0.5 * mag).to(BF16)
    r = (torch.randn(N, generator=g) * mag).to(BF16)
    return (b if bias else None), (r if res else None)


def activation_row(gen, K, fused, seed=0):
    """-> (x bf16 (K,), gain bf16 (K,) or None).  Fused kernels: x at scale 2.5 and a gain over a decade (bits: x is the probe, gain 1)."""
    g = _gen(3000 + seed + K)
    if not fused:
        return torch.randn(K, generator=g).to(BF16), None
    return (torch.randn(K, generator=g) * 2.5).to(BF16), torch.pow(10.0, torch.rand(K, generator=g) - 0.5).to(BF16)


def pad_rows(family, o, pad_vecs=1):
    """The weight matrix as a column slice [:, :cols] of a wider tensor whose pad columns hold the largest finite values, so that a
    kernel that indexes rows by K instead of the row stride, or reads past K, is far off.  Returns the strided view."""
    if family == "bf16":
        W = o["W"]
        wide = torch.full((W.shape[0], W.shape[1] + 8 * pad_vecs), 3.0e38, dtype=BF16, device=W.device)
        wide[:, :W.shape[1]] = W
        return wide[:, :W.shape[1]]
    if family == "fp8":
        W = o["W8"].view(torch.uint8)
        wide = torch.full((W.shape[0], W.shape[1] + 16 * pad_vecs), 0x7E, dtype=torch.uint8, device=W.device)          # 448
        wide[:, :W.shape[1]] = W
        return wide.view(torch.float8_e4m3fn)[:, :W.shape[1]]
    W = o["W4"]
    wide = torch.full((W.shape[0], W.shape[1] + 16 * pad_vecs), 0x77, dtype=torch.uint8, device=W.device)              # 6.0, 6.0
    wide[:, :W.shape[1]] = W
    return wide[:, :W.shape[1]]


# ------------------------------------------------------------------------------------------------ the case list
QKV_D128 = dict(D=128, Hq=1, Hkv=1)          # N = 384
QKV_D37 = dict(D=37, Hq=3, Hkv=1)            # N = 185: ragged


def _case(family, kind, N, K, gens, bias=False, res=False, f32=False, inplace=False, act=0, pad=False, qkv=None, tag=""):
    if kind == "qkv":                                  # the bias is not optional; no residual, one output type
        qkv = qkv or QKV_D37
        N = (qkv["Hq"] + 2 * qkv["Hkv"]) * qkv["D"]
        bias, res = True, False
    elif kind != "gemv":
        bias = res = False
    f = form(family, kind, N, K)
    opts = "".join(s for s, on in (("+b", bias and kind != "qkv"), ("+r", res), ("+f32", f32), ("+inpl", inplace), (f"+act{act}", act),
                                   ("+pad", pad), (f"+D{qkv['D']}" if qkv else "", bool(qkv))) if on)
    return dict(id=f"{f['name']}-N{N}-K{K}-{'.'.join(gens)}{opts}{tag}", family=family, kind=kind, N=N, K=K, gens=tuple(gens), bias=bias,
                res=res or inplace, f32=f32, inplace=inplace, act=act, pad=pad, qkv=qkv, form=f)


def _edge_ks(family, kind, N_of):
    """For every form of (family, kind) the product reaches: the Ks of its ragged-edge conditions, smallest first."""
    vec = VEC[family]
    want, first = {}, {}
    for N in N_of:
        kmax = 19008 if kind == "gemv" else FUSED_MAX_K
        for K in range(vec, kmax + 1, vec):
            f = form(family, kind, N, K)
            for c in k_conditions(f, K):
                want.setdefault((form_key(f), c), (N, K))
            first.setdefault(form_key(f), (N, K))
    for key, nk in first.items():                      # a form that admits none of the conditions: its shortest row
        if not any(k[0] == key for k in want):
            want[(key, "reached")] = nk
    return want


def build_cases():
    cases = []
    alt = 0
    for family in FAMILIES:
        for kind in KINDS[family]:
            # N = 133 (1 row per wave, and the K-split form from K = 4096), 4099 / 8195 (2 rows), 16387 (4 rows): never a multiple of
            # the rows of a workgroup, so every case checks the clamped rows and the sentinels behind the output
            n_of = (133, 4099, 8195, 16387) if kind == "gemv" else (133,)
            picked = {}
            for (key, cond), (N, K) in sorted(_edge_ks(family, kind, n_of).items(), key=lambda kv: (kv[1][0], kv[1][1])):
                picked.setdefault((N, K), []).append(cond)
            seen_forms = set()
            for (N, K) in picked:                      # the first case of a form runs all three generators, the others alternate
                alt += 1
                key = form_key(form(family, kind, N, K))
                gens = ("bits", "spread" if alt % 2 else "iid") if key in seen_forms else ("bits", "iid", "spread")
                seen_forms.add(key)
                cases.append(_case(family, kind, N, K, gens, bias=alt % 3 != 0, res=alt % 2 == 0))
        # two rows per wave with a row longer than 4096 needs N > 8192 (below, K >= 4096 is the K-split form)
        cases.append(_case(family, "gemv", 8195, 4096 + VEC[family], ("bits",), bias=True, res=True))
    for family in FAMILIES:
        # model shapes: o_proj and down_proj of Qwen2-VL-2B (1536, 8960) and 7B (3584, 18944)
        for (N, K) in ((1536, 1536), (1536, 8960), (3584, 3584), (3584, 18944)):
            cases.append(_case(family, "gemv", N, K, ("iid", "spread"), res=True, inplace=True, tag="-model"))
        # the epilogue's operand combinations, N = 1, the padded row stride
        cases.append(_case(family, "gemv", 133, 1024 + VEC[family], ("spread",), bias=True))
        cases.append(_case(family, "gemv", 133, 1024 + VEC[family], ("spread",), res=True))
        cases.append(_case(family, "gemv", 133, 1024 + VEC[family], ("bits", "spread"), bias=True, res=True, f32=True))
        cases.append(_case(family, "gemv", 133, 4096 + 4 * VEC[family], ("bits", "spread"), bias=True, res=True, f32=True))
        cases.append(_case(family, "gemv", 133, 4096 + 5 * VEC[family], ("bits", "spread"), bias=True, inplace=True))
        cases.append(_case(family, "gemv", 1, 1024 + VEC[family], ("iid",), bias=True, res=True))
        cases.append(_case(family, "gemv", 1, 4096 + VEC[family], ("iid",), bias=True, res=True))
        cases.append(_case(family, "gemv", 133, 1024 + VEC[family], ("bits", "spread"), bias=True, res=True, pad=True))
        cases.append(_case(family, "gemv", 133, 4096 + 3 * VEC[family], ("bits", "spread"), bias=True, res=True, pad=True))
        cases.append(_case(family, "gemv", 4099, 1024 + VEC[family], ("bits",), bias=True, res=True, pad=True))
        for kind in KINDS[family][1:]:
            cases.append(_case(family, kind, 133, 1536 + 32, ("bits", "spread"), pad=True))
            if kind != "qkv":
                cases.append(_case(family, kind, 1, 2048 + 32, ("iid",)))
        cases.append(_case(family, "qkv", 0, 2048, ("bits", "iid"), qkv=QKV_D128))
    for act in (ACT_QUICK_GELU, ACT_GELU_ERF, ACT_SILU):
        cases.append(_case("bf16", "gemv", 133, 1032, ("iid", "spread"), bias=True, res=True, act=act))
        cases.append(_case("bf16", "gemv", 133, 4104, ("spread",), bias=True, res=True, act=act))
    seen, out = set(), []
    for c in cases:                 # the same (shape, options) can come out of two rules: keep the first
        if c["id"] not in seen:
            seen.add(c["id"])
            out.append(c)
    return out


CASES = build_cases()
