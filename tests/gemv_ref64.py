"""fp64 reference and per-element error bound for the decode GEMV path tests (test helper, not product).

Reference.  From the SAME operands the kernel gets -- bf16 weights, or e4m3 codes with fp32 row scales, or e2m1 codes with e8m0 block
scales, dequantised EXACTLY to W' (tests/gemv_paths.py:weights keeps W' in float32, which holds every one of them) -- in float64:
    z = W' . x (+ bias)            E = |W'| . |x| + |bias|       then the epilogue of each kernel as its code rounds it.

Products are exact in fp32 in all three families, so only additions round: a bf16 activation has 8 significant bits, a bf16 weight 8
(16-bit product), an e4m3 code 4 (12 bits), an e2m1 code 2 (10 bits); the fp4 block scale is a power of two that the conversion
multiplies into the code exactly, and the fp8 row scale is applied once to the finished sum.  All fit fp32's 24 bits.

Summation term  S = c u24 E,  u24 = 2^-24: c is the number of fp32 additions a product can pass through on its way to the output,
whatever the order inside, read off the kernels (gemv.hip, decode_fused.hip, decode_fp8.hip, decode_fp4.hip):
    c = VEC * steps + 6 + (KW - 1) + [bias] + [fp8]
  VEC * steps  the per-lane FMA chain: VEC = 8 (bf16) / 16 (fp8) / 32 (fp4) products for each K-step the lane executes; a lane executes
               steps = PRE * ceil(span / (PRE * 64 VEC)) K-steps (whole pre-issued batches; a masked step adds an exact zero), span = K,
               or the K / KW share of a wave in the K-split forms
  6            the wave_sum butterfly (four DPP steps inside a 16-lane row, permlane16 and permlane32 swaps)
  KW - 1       the K-split partials summed by one thread (KW = 4: gemv_bf16_ksplit_kernel, gemv_fp8_kernel<2, 4, 3>, gemv_fp4_kernel<2, 4, 2>)
  [bias]       acc + bias: 1 where the kernel has a bias
  [fp8]        acc * scale: 1 in the fp8 family (exact for the power-of-two scales the product makes; counted because the ABI takes any)
  forms: bf16 gemv 1 row PRE 4, 2 rows PRE 4, 4 rows PRE 3, K-split 2 rows PRE 5; fp8 gemv 1 row PRE 4, 2 / 4 rows PRE 2, K-split PRE 3;
  fp4 gemv 1 / 2 rows PRE 1 (K <= 2048) or 2, K-split PRE 2; fused kernels PRE by DEC_DISPATCH / DEC8_DISPATCH / DEC4_DISPATCH.

Epilogues (u8 = 2^-8: one round-to-nearest to bf16 moves v by at most u8 |v|); dz = S + u8 (|z| + S) is gemm_ref64's "Linear output":
  plain GEMV   v = rbf(acc [* scale] + bias): dz.  apply_act(v) -> gemm_ref64._rounded_act.  rbf(v + residual): one fp32 addition and
               one rounding, d = da + u24 |y|, bound = d + u8 (|y| + d).  Stored as bf16, or as fp32 that must be bf16-representable.
  dec_qkv*     bf16(acc [* scale] + bias): dz.
  dec_gate_up* g = rbf(acc_g), u = rbf(acc_u): dz each; sg = rbf(silu(g)) -> _rounded_act; y = bf16(sg u): the SwiGLU branch of
               gemm_ref64.reference.
  dec_lm_head* rbf(acc [* scale]) into fp32 logits: dz.
The bound is derived, not tuned: the tests hold err / bound <= 1 on every element and mean (err / bound) <= MEAN_TOL (gemm_ref64).

Norm prologue (dec_xrow.h).  The reference of a fused kernel is the fp64 GEMV of the kernel's OWN staged row xs, so the norm's
roundings are not counted twice and no near-tie is guessed: xs is recovered bit for bit by running an entry point of the same family
with an identity weight matrix (dec_lm_head* with W = I writes logits[n] = xs[n]; fp4, which has no head, through dec_qkv_fp4 with a
zero bias), and is itself checked against the fp64 RMSNorm of x under gemm_ref64.norm_reference's RMS bound.

`bits` operands need no bound: every partial sum is an integer multiple of 2^-4 below 2^24 of them, so fp32 accumulates exactly in any
order and the output is the exact value passed through the epilogue's roundings: bit equality (dec_gate_up*: silu is not exact, the
output is held to the SwiGLU epilogue bound alone, c = 0).

Observed worst / mean err / bound: on the CPU (tests/test_gemv_ref64.py) the bf16 oracle reaches 0.54 / 0.12 with c = K + 1 and the fp32
emulation of the forms 0.76 / 0.21 with the forms' own c.  The MI355X figures per family and form are printed by every case of
tests/test_gemv_paths_gpu.py (`[gemv-path] <form> <generator> ... worst err/bound .. mean ..`); they have not been recorded here yet.
"""
from __future__ import annotations

import torch

from gemm_ref64 import MEAN_TOL, U8, U24, _rounded_act, check, norm_reference, ratios  # noqa: F401  (re-exported to the tests)

BF16 = torch.bfloat16
ACT_NONE, ACT_SILU = 0, 3
_BLOCK_ROWS = 1024


def fadds(form, bias):
    """c of the module docstring for a form of gemv_paths.form()."""
    span = max(hi - lo for lo, hi in form["ranges"])
    steps = form["pre"] * max(1, -(-span // form["batch"]))
    return form["vec"] * steps + 6 + (form["kw"] - 1) + (1 if bias else 0) + (1 if form["family"] == "fp8" else 0)


def dot64(Wf, x):
    """(W' . x, |W'| . |x|) in float64, blocked over rows; Wf (N, K) float32 holding W' exactly, x (K,) bf16.  Runs where Wf lives."""
    xd = x.to(Wf.device).double()
    xa = xd.abs()
    z = torch.empty(Wf.shape[0], dtype=torch.float64, device=Wf.device)
    E = torch.empty_like(z)
    for r0 in range(0, Wf.shape[0], _BLOCK_ROWS):
        w = Wf[r0:r0 + _BLOCK_ROWS].double()
        z[r0:r0 + _BLOCK_ROWS] = w @ xd
        E[r0:r0 + _BLOCK_ROWS] = w.abs() @ xa
    return z.cpu(), E.cpu()


def rbf64(t):
    """One round-to-nearest-even to bf16 of a float64 tensor whose values fp32 holds exactly (the `bits` sums)."""
    f = t.float()
    assert torch.equal(f.double(), t), "rbf64: the value does not fit fp32, the double rounding would not be the kernel's single one"
    return f.to(BF16).double()


def reference(kind, Wf, x, c, bias=None, residual=None, act=ACT_NONE):
    """-> (y, bound) float64 (N,) on the CPU.  kind: gemv | qkv | gate_up (Wf = [gate rows; up rows]) | lm_head.  x: the row the dot
    products see (the fused kernels: the staged xs).  c: fadds(form, bias)."""
    z, E = dot64(Wf, x)
    if bias is not None:
        z = z + bias.cpu().double()
        E = E + bias.cpu().double().abs()
    S = c * U24 * E
    dz = S + U8 * (z.abs() + S)
    if kind in ("qkv", "lm_head"):
        assert residual is None and act == ACT_NONE
        return z, dz
    if kind == "gate_up":
        I = z.shape[0] // 2
        g, u, dg, du = z[:I], z[I:], dz[:I], dz[I:]
        sg, dsg = _rounded_act(g, dg, ACT_SILU)
        y = sg * u
        d = u.abs() * dsg + sg.abs() * du + dsg * du + U24 * y.abs()
        return y, d + U8 * (y.abs() + d)
    assert kind == "gemv", kind
    a, da = _rounded_act(z, dz, act)
    if residual is None:
        return a, da
    y = a + residual.cpu().double()
    d = da + U24 * y.abs()
    return y, d + U8 * (y.abs() + d)


def bits_reference(kind, Wf, x, bias=None, residual=None):
    """The exact output for `bits` operands: -> (y, bound or None).  bound None: y is exact, compare bit for bit."""
    z, E = dot64(Wf, x)
    assert float(E.max()) * 16 < 2 ** 24 and torch.equal(z * 16, (z * 16).round()), "bits: partial sums must be multiples of 2^-4 below 2^20"
    if kind == "gate_up":
        return reference(kind, Wf, x, 0)
    if bias is not None:
        z = z + bias.cpu().double()
    y = rbf64(z)
    if residual is not None:
        y = rbf64(y + residual.cpu().double())
    return y, None


def xs_reference(x, gain, eps):
    """fp64 RMSNorm of x and the RMS bound of gemm_ref64.norm_reference -> (xs, bound) float64 (K,)."""
    xn, bound = norm_reference(x.reshape(1, -1), gain, None, eps)
    return xn[0], bound[0]


def where_rows(bad_rows, form):
    """Name failing rows for the kernel author: the rows, their position inside the rows-per-wave group, the wave, the workgroup."""
    r, wg = form["rows"], form["wg_rows"]
    rows = [int(n) for n in bad_rows[:16]]
    pos = sorted(set(n % r for n in (int(b) for b in bad_rows)))
    waves = sorted(set((n % wg) // r for n in (int(b) for b in bad_rows)))
    wgs = sorted(set(n // wg for n in (int(b) for b in bad_rows)))
    return (f"form {form['name']} ({r} rows per wave, {wg} per workgroup, KW {form['kw']}, PRE {form['pre']}, XC {form['xc']}, K ranges "
            f"{form['ranges']}): {len(bad_rows)} rows off, rows {rows}{'...' if len(bad_rows) > 16 else ''}; position in the wave's row group "
            f"{pos}; row group of the workgroup {waves}; workgroups {wgs[:12]}{'...' if len(wgs) > 12 else ''}")


def check_rows(name, got, ref, bound, form, n_out=None):
    """gemm_ref64.check (bound None: bit equality), naming the rows, their place in the wave and the kernel form on failure.
    n_out: rows of the OUTPUT (gate_up: I) for the row naming."""
    try:
        g2, r2 = got.reshape(1, -1), ref.reshape(1, -1)             # check() names (row, column) tiles: one row of N columns
        if bound is None:
            return check(name, g2, r2, torch.ones_like(r2), exact=True)
        return check(name, g2, r2, bound.reshape(1, -1))
    except AssertionError as e:
        g = got.detach().cpu().double().reshape(ref.shape)
        bad = ((g != ref) if bound is None else ((g - ref).abs() > bound) | ~torch.isfinite(g)).nonzero().reshape(-1)
        if bad.numel() == 0:
            raise
        raise AssertionError(f"{e}\n    {where_rows(bad, form)}") from None


# ------------------------------------------------------------------------------------------------ fp32 emulation of a form (CPU)
def _rbf(t):
    return t.to(BF16).float()


def _apply_act32(y, act):
    """common.h:apply_act in fp32 (y is bf16-rounded)."""
    if act == 1:
        t = _rbf(1.702 * y)
        return _rbf(y * _rbf(1.0 / (1.0 + torch.exp(-t))))
    if act == 2:
        return _rbf(0.5 * y * (1.0 + torch.erf(y * 0.70710678118654752440)))
    if act == 3:
        return _rbf(y / (1.0 + torch.exp(-y)))
    return y


def emulate_dots(form, Wq, x, shift_wave=None):
    """acc[r] of one launch in fp32, in the kernel's order: per lane the FMA chain over its VEC elements of every K-step of every
    batch (a lane past the wave's range loads a clamped address and multiplies by zero), the wave_sum butterfly, the KW partials
    left to right.  Wq (R, K) float32, x (K,) bf16.  shift_wave: (wave, vectors) moves that wave's K range (an injected fault)."""
    vec, step, pre, batch = form["vec"], form["step"], form["pre"], form["batch"]
    K = Wq.shape[1]
    xf = x.float()
    lane = torch.arange(64)
    parts = []
    for p, (lo, hi) in enumerate(form["ranges"]):
        if shift_wave is not None and shift_wave[0] == p:
            lo, hi = lo + shift_wave[1] * vec, min(K, hi + shift_wave[1] * vec)
        acc = torch.zeros((Wq.shape[0], 64), dtype=torch.float32)
        for base in range(lo, hi, batch):
            for it in range(pre):
                c = base + it * step + lane * vec
                inr = c < hi
                idx = torch.where(inr, c, torch.full_like(c, lo))[:, None] + torch.arange(vec)[None, :]
                xv = xf[idx] * inr[:, None].float()
                wv = Wq[:, idx]
                for i in range(vec):
                    acc = acc + wv[:, :, i] * xv[None, :, i]          # the product is exact in fp32: one rounding, as fmaf
        for o in (1, 2, 4, 8, 16, 32):
            acc = acc + acc[:, lane ^ o]
        parts.append(acc[:, 0])
    s = parts[0]
    for q in parts[1:]:
        s = s + q
    return s


def emulate(form, Wq, x, scale=None, bias=None, residual=None, act=ACT_NONE, drop_rbf=False, shift_wave=None):
    """One launch in fp32 with the epilogue of its kind -> float32 (N,) holding the stored values.  scale: the fp8 row scales (Wq = the
    codes as float).  drop_rbf: leave out the rounding of the Linear output (an injected fault)."""
    acc = emulate_dots(form, Wq, x, shift_wave)
    if scale is not None:
        acc = acc * scale.float()
    kind = form["kind"]
    rb = (lambda t: t) if drop_rbf else _rbf
    if kind == "gate_up":
        I = acc.shape[0] // 2
        return _rbf(_apply_act32(rb(acc[:I]), 3) * rb(acc[I:]))
    if bias is not None:
        acc = acc + bias.float()
    if kind in ("qkv", "lm_head"):
        return rb(acc)
    v = _apply_act32(rb(acc), act)
    if residual is not None:
        v = _rbf(v + residual.float())
    return _rbf(v)
