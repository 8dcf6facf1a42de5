"""fp64 GEMM reference and per-element error bound for the GEMM path tests (test helper, not product).

Reference.  From the SAME bf16 (or e4m3 codes + fp32 scales) operands the kernel gets, in float64:
    z = A . W^T + bias          y = act(z) (+ residual)          SwiGLU: y = silu(z_gate) * z_up
    E = |A| . |W|^T + |bias|    (the magnitude fp32 summation error scales with; computed in fp32, it is only a scale)

Bound, per output element, read off the epilogues of csrc/gemm.hip (u8 = 2^-8: bf16 keeps 8 significant bits, so ONE
round-to-nearest moves a value v by at most half an ulp <= 2^-8 |v|; u24 = 2^-24 likewise for fp32):

  fp32 summation  S = c * u24 * E.  bf16 x bf16 and e4m3 x e4m3 products are exact in fp32, so only additions round.  c is the
      largest number of fp32 additions any product passes through on its way to the output (the classical bound for a
      summation tree of that depth, whatever the order inside): at most 32 inside the MFMA block that takes the product in
      (v_mfma_f32_16x16x32_bf16 sums 32 products per output; the fp8 16x16x128 form sums 128), + ceil(kps / 32) additions along
      the accumulator chain of one K-split (kps / 128 for fp8), + (splits - 1) in the split-K reduce, + 1 for the bias:
          c = block + ceil(kps / block) + splits          (block = 32 for bf16, 128 for fp8)
      The fp8 GEMM multiplies the accumulator by sa[m] * sw[n] (two more fp32 roundings): c + 2 there.
  Linear output   z_b = bf16(acc + bias):                     dz = S + u8 (|z| + S)
  activation      a_b = act(z_b), evaluated in fp32 and rounded to bf16 as the eager module does (common.h: apply_act):
      silu, gelu(erf): one rounding.   da = |act'(z)| dz + C2/2 dz^2 + 8 u24 (|z| + |a|) + u8 (|a| + all of that)
                       (Taylor with the activation's own slope at z; C2 = max |act''| = 0.5 silu, 0.8 gelu; 8 u24 (..) covers the
                       fp32 evaluation: every intermediate is bounded by |z| and there are fewer than 8 operations)
      quick_gelu: three roundings, t = bf16(1.702 z_b), s = bf16(sigmoid(t)), a = bf16(z_b s): propagated one by one the same way.
  residual        y = bf16(a_b + r): one fp32 addition and the final rounding:  dy = da + u24 |y| + u8 (|y| + da)
      (without residual the final store rounds a bf16 value to bf16: no error)
  SwiGLU          g_b, u_b as "Linear output"; sg = bf16(silu(g_b)) as "activation"; y = bf16(sg * u_b):
                  dy = |u| dsg + |sg| du + dsg du + u24 |y| + u8 (|y| + all of that)
The bound is derived, not tuned; the tests hold err / bound <= 1 on every element.

Mean bound.  A round-to-nearest error is uniform over [-1/2, 1/2] ulp, mean magnitude 1/4 ulp = HALF the per-element bound of that
rounding, so a correct kernel has mean (err / bound) <= 1/2 whatever the data (observed 0.2-0.36); an error of 0.65 roundings added
to every element lifts the mean over 1/2.  MEAN_TOL = 0.5.

Fused norm outputs (svlm_gemm_bf16_norm, svlm_gemm_fp8 with a norm): reference = fp64 norm of the KERNEL'S OWN bf16 GEMM output, so
the GEMM's roundings are not counted twice.  RMSNorm  xn = bf16(g * bf16(y r)):  u8 |g y r| (1 + u8) + u8 |xn| + (N + 4) u24 |xn|
(r from an fp32 sum of N squares and rsqrtf).  LayerNorm  xn = bf16((y - mean) rstd g + h), one rounding:
u8 |xn| + |g| rstd (N u24 mean|y|) + (N + 4) u24 |xn - h| + 4 u24 (|xn| + |h|).
"""
from __future__ import annotations

import math

import torch

U8 = 2.0 ** -8
U24 = 2.0 ** -24
MEAN_TOL = 0.5
ACT_NONE, ACT_QUICK_GELU, ACT_GELU_ERF, ACT_SILU, ACT_SWIGLU = 0, 1, 2, 3, 4
_BLOCK_ROWS = 256                         # rows of A per fp64 matmul block: (256, N) doubles at N = 18944 are 39 MB


def matmul64(A, W, small_ints=False):
    """(A . W^T in float64, |A| . |W|^T in float32 -> float64), blocked over rows of A.  small_ints: the operands are small integers
    whose every partial sum stays below 2^24 (the exact / rowcol generators), so a float32 product IS the exact result."""
    M = A.shape[0]
    if small_ints:
        Wa = W.float().t().contiguous()
        z, E = A.float() @ Wa, A.float().abs() @ Wa.abs()
        assert float(E.max()) < 2 ** 24
        return z.double(), E.double()
    Wd, Wa = W.double().t().contiguous(), W.float().abs().t().contiguous()
    z = torch.empty((M, W.shape[0]), dtype=torch.float64)
    E = torch.empty((M, W.shape[0]), dtype=torch.float64)
    for r0 in range(0, M, _BLOCK_ROWS):
        r1 = min(M, r0 + _BLOCK_ROWS)
        z[r0:r1] = A[r0:r1].double() @ Wd
        E[r0:r1] = (A[r0:r1].float().abs() @ Wa).double()
    return z, E


def fadds(plan, K):
    """c of the module docstring for a plan dict (keys fp8, splits, kps)."""
    block = 128 if plan.get("fp8") else 32
    kps = plan["kps"] if plan["splits"] > 1 else K
    return block + (kps + block - 1) // block + plan["splits"] + (2 if plan.get("fp8") else 0)


def _sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def _act64(z, act):
    """-> (act(z), |act'(z)|, max |act''|) in float64."""
    if act == ACT_SILU:
        s = _sigmoid(z)
        return z * s, (s + z * s * (1 - s)).abs(), 0.5
    if act == ACT_GELU_ERF:
        phi = torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)
        Phi = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
        return z * Phi, (Phi + z * phi).abs(), 0.8
    raise ValueError(act)


def _rounded_act(z, dz, act):
    """act(z_b) rounded to bf16 as apply_act does -> (fp64 value at z, error bound given |z_b - z| <= dz)."""
    if act == ACT_NONE:
        return z, dz
    if act in (ACT_SILU, ACT_GELU_ERF):
        a, slope, c2 = _act64(z, act)
        d = slope * dz + 0.5 * c2 * dz * dz + 8 * U24 * (z.abs() + a.abs())
        return a, d + U8 * (a.abs() + d)
    if act == ACT_QUICK_GELU:
        t = 1.702 * z
        dt = 1.702 * dz + U24 * t.abs()
        dt = dt + U8 * (t.abs() + dt)                                  # t = bf16(1.702 z_b)
        s = _sigmoid(t)
        ds = s * (1 - s) * dt + 0.5 * 0.0963 * dt * dt + 4 * U24       # sigmoid'' <= 0.0963; expf, add, divide in fp32
        ds = ds + U8 * (s + ds)                                        # s = bf16(sigmoid(t))
        a = z * s
        d = z.abs() * ds + s * dz + dz * ds + U24 * a.abs()
        return a, d + U8 * (a.abs() + d)                               # a = bf16(z_b s)
    raise ValueError(act)


def reference(A, W, bias=None, residual=None, act=ACT_NONE, c=None, a_scale=None, w_scale=None, small_ints=False):
    """-> (y, bound, z, E): float64 (M, N) each.  A (M, K), W (N, K) [SwiGLU: (2N, K) = gate rows; up rows], bias (N,) [(2N,)],
    residual (M, N).  a_scale / w_scale: fp8 GEMM, A and W hold the dequantised-to-float CODES and the scales multiply z.
    c: fp32 additions per output (fadds(plan, K))."""
    assert c is not None
    z, E = matmul64(A, W, small_ints)
    if a_scale is not None:
        sc = a_scale.double()[:, None] * w_scale.double()[None, :]
        z, E = z * sc, E * sc
    if bias is not None:
        z = z + bias.double()[None, :]
        E = E + bias.double().abs()[None, :]
    S = c * U24 * E
    dz = S + U8 * (z.abs() + S)
    if act == ACT_SWIGLU:
        I = z.shape[1] // 2
        g, u, dg, du = z[:, :I], z[:, I:], dz[:, :I], dz[:, I:]
        sg, dsg = _rounded_act(g, dg, ACT_SILU)
        y = sg * u
        d = u.abs() * dsg + sg.abs() * du + dsg * du + U24 * y.abs()
        return y, d + U8 * (y.abs() + d), z, E
    a, da = _rounded_act(z, dz, act)
    if residual is None:
        return a, da, z, E
    y = a + residual.double()
    d = da + U24 * y.abs()
    return y, d + U8 * (y.abs() + d), z, E


def norm_reference(y_kernel, norm_w, norm_b, eps):
    """fp64 norm of the kernel's own bf16 GEMM output -> (xn, bound)."""
    y = y_kernel.detach().cpu().double()
    g = norm_w.detach().cpu().double()[None, :]
    N = y.shape[1]
    if norm_b is None:
        r = torch.rsqrt((y * y).mean(dim=1, keepdim=True) + eps)
        xn = g * y * r
        return xn, U8 * (g * y * r).abs() * (1 + U8) + U8 * xn.abs() + (N + 4) * U24 * xn.abs()
    h = norm_b.detach().cpu().double()[None, :]
    mean = y.mean(dim=1, keepdim=True)
    rstd = torch.rsqrt(((y - mean) ** 2).mean(dim=1, keepdim=True) + eps)
    xn = (y - mean) * rstd * g + h
    bound = U8 * xn.abs() + g.abs() * rstd * (N * U24 * y.abs().mean(dim=1, keepdim=True)) + (N + 4) * U24 * (xn - h).abs() \
        + 4 * U24 * (xn.abs() + h.abs())
    return xn, bound * (1 + U8)


def ratios(got, ref, bound):
    """-> (err / bound per element, mean err / bound); got is cast to float64."""
    err = (got.detach().cpu().double().reshape(ref.shape) - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where((err == 0), torch.zeros_like(ratio), ratio)
    return ratio, float(ratio.mean())


def _where(ratio, plan, K, swiglu):
    """Tile rows / tile columns / K-splits over the bound, for the tile author.  A failing (m, n) names its tile directly; the K-split
    cannot be read off one output, so it is named when the failing set is what ONE split's slab would cause (every element of
    whole tiles) and listed as 'any of s splits' otherwise."""
    bm = plan.get("bm") or 64
    bn = 64 if swiglu else 128
    bad = (ratio > 1.0).nonzero()
    tm = sorted(set((bad[:, 0] // bm).tolist()))
    tn = sorted(set((bad[:, 1] // bn).tolist()))
    rows16 = sorted(set((bad[:, 0] // 16).tolist()))
    s = plan.get("splits", 1)
    ksplit = "unsplit" if s <= 1 else f"any of {s} splits of {plan.get('kps')} k (kps does not show in one output)"
    return (f"{bad.shape[0]} elements over the bound; tile rows (of {bm}) {tm[:12]}{'...' if len(tm) > 12 else ''}, tile columns (of {bn}) "
            f"{tn[:12]}{'...' if len(tn) > 12 else ''}, 16-row fragments {rows16[:12]}{'...' if len(rows16) > 12 else ''}; K: {ksplit}")


def check(name, got, ref, bound, plan=None, K=0, swiglu=False, exact=False):
    """Assert the per-element bound and the mean bound (exact=True: bit equality with the reference, which must then be exactly
    representable); print the worst ratios (1.0 = at the limit) and where; on failure say which tiles are over."""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (name, tuple(got.shape), tuple(ref.shape))
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    plan = plan or {}
    if exact:
        ne = got.double() != ref
        n_bad = int(ne.sum())
        print(f"[{name}] exact: {n_bad} of {ne.numel()} elements differ")
        if n_bad:
            idx = [int(i) for i in ne.nonzero()[0]]
            raise AssertionError(f"{name}: {n_bad} elements differ from the exact reference, first at {idx} (got "
                                 f"{float(got[tuple(idx)]):.6g}, ref {float(ref[tuple(idx)]):.6g}); "
                                 + _where(ne.double() * 2, plan, K, swiglu))
        return 0.0, 0.0
    ratio, mean = ratios(got, ref, bound)
    worst = float(ratio.max())
    idx = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
    print(f"[{name}] worst err/bound={worst:.3f} at {idx} mean err/bound={mean:.3f}")
    if worst > 1.0:
        raise AssertionError(f"{name}: err/bound {worst:.3f} > 1 at {idx} (got {float(got[tuple(idx)]):.6g}, ref {float(ref[tuple(idx)]):.6g}, "
                             f"bound {float(bound[tuple(idx)]):.3g}); " + _where(ratio, plan, K, swiglu))
    assert mean <= MEAN_TOL, f"{name}: mean err/bound {mean:.3f} > {MEAN_TOL}"
    return worst, mean
