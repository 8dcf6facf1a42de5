"""fp64 attention reference for the split / merge tests (test helper, not product).

The kernels rotate q and K to bf16 first (RoPE-on-load, bit-identical to RefOps._rot), then compute softmax(q.K^T * scale).V with
fp32 scores, P rounded to bf16 before P.V and fp32 accumulation, and round the output to bf16.  attend64 takes the SAME bf16 rotated
inputs and does everything after them in float64 with no rounding of P, so it states what attention is independently of the
kernels' (and oracle.model.flash_attention's) design choices.

Bound held by the tests, per output element:  |out - ref| <= 2^-8 * E + 2^-8 * |ref|,  E = (sum_j p_j |v_j|) / sum_j p_j.
bf16 keeps 8 significant bits, so one rounding moves a value by at most 2^-8 of itself (2^-9 of it on average over the binade):
rounding every P entry moves the output by at most 2^-8 * E (all errors aligned, which random data never reaches), rounding the output
by at most 2^-8 * |ref|.  A merge that gives one split a wrong weight moves the output by the order of that split's share of E.
Mean bound: mean |out - ref| / (E + |ref|) <= 2^-10.
"""
from __future__ import annotations

import torch

TOL = 2.0 ** -8
MEAN_TOL = 2.0 ** -10
_ROWS_PER_BLOCK_ELEMS = 1 << 24          # scores held at once: 16M doubles = 128 MB


def attend64(q_rot, K_rot, V, causal_offset, scale):
    """q_rot (Hq, T, D), K_rot / V (Hkv, L, D): bf16 (or any dtype; promoted to float64).  Query head h attends with kv head
    h // (Hq // Hkv).  causal_offset None: every query sees every key; else query row i sees keys j <= causal_offset + i.
    Works per kv head with the group's query heads stacked (no GQA-expanded copy of K / V).
    Returns (out, E), both (Hq, T, D) float64."""
    Hq, T, D = q_rot.shape
    Hkv, L, _ = K_rot.shape
    assert V.shape == K_rot.shape and Hq % Hkv == 0
    G = Hq // Hkv
    out = torch.empty((Hq, T, D), dtype=torch.float64)
    E = torch.empty((Hq, T, D), dtype=torch.float64)
    rows_blk = max(1, _ROWS_PER_BLOCK_ELEMS // max(L, 1))
    for h in range(Hkv):
        K = K_rot[h].double()
        Vh = V[h].double()
        Va = Vh.abs()
        Q = q_rot[h * G:(h + 1) * G].double().reshape(G * T, D)      # row r = g * T + t
        for r0 in range(0, G * T, rows_blk):
            r1 = min(G * T, r0 + rows_blk)
            S = (Q[r0:r1] @ K.t()) * float(scale)
            if causal_offset is not None:
                t = torch.arange(r0, r1) % T
                S.masked_fill_(torch.arange(L)[None, :] > (t[:, None] + causal_offset), float("-inf"))
            P = torch.exp(S - S.max(dim=1, keepdim=True).values)
            l = P.sum(dim=1, keepdim=True)
            o = (P @ Vh) / l
            e = (P @ Va) / l
            out[h * G:(h + 1) * G].view(G * T, D)[r0:r1] = o
            E[h * G:(h + 1) * G].view(G * T, D)[r0:r1] = e
    return out, E


def bound_ratios(got, ref, E):
    """-> (err / bound per element, mean |err| / (E + |ref|) / MEAN_TOL); got is cast to float64."""
    err = (got.detach().cpu().double() - ref).abs()
    bound = TOL * (E + ref.abs())
    ratio = err / bound.clamp_min(1e-300)
    mean = float((err / (E + ref.abs()).clamp_min(1e-300)).mean()) / MEAN_TOL
    return ratio, mean


def check(name, got, ref, E):
    """Assert the per-element and the mean bound; print the worst observed ratios (1.0 = at the limit) so the margin shows."""
    got = got.detach().cpu().reshape(ref.shape)
    assert torch.isfinite(got.float()).all(), f"{name}: non-finite output"
    ratio, mean = bound_ratios(got, ref, E)
    worst = float(ratio.max())
    idx = [int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]
    print(f"[{name}] worst err/bound={worst:.3f} at {idx} mean err/(E+|ref|)={mean:.3f} x 2^-10")
    if worst > 1.0:
        # which heads are off, and by how much (a wrongly weighted split shows up on every column of the heads it feeds)
        per_head = ratio.reshape(ratio.shape[0], -1).amax(dim=1)
        bad = [(h, round(float(v), 2)) for h, v in enumerate(per_head.tolist()) if v > 1.0]
        raise AssertionError(f"{name}: err/bound {worst:.3f} > 1 at {idx} (got {float(got.reshape(ref.shape)[tuple(idx)]):.6g}, "
                             f"ref {float(ref[tuple(idx)]):.6g}, E {float(E[tuple(idx)]):.6g}); heads over the bound: {bad}")
    assert mean <= 1.0, f"{name}: mean err/(E+|ref|) {mean:.3f} x 2^-10 > 2^-10"
    return worst, mean
