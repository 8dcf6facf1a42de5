"""Weight containers: HF state-dict names in, device-resident fused bf16 matrices out.

State-dict keys follow ``Qwen2VLForConditionalGeneration`` (transformers >= 4.52 layout, the one
the reference patches: ``model.model.language_model`` / ``model.model.visual``,
qwen2/patch_model.py:24-26), so ``convert_qwen2_to_streaming(hf_model)`` can pass
``hf_model.state_dict()`` straight in.
"""
from __future__ import annotations

from typing import Dict

import torch

from .config import ModelConfig

V_PREFIX = "model.visual."
L_PREFIX = "model.language_model."


def state_dict_shapes(cfg: ModelConfig) -> Dict[str, tuple]:
    vc, tc = cfg.vision, cfg.text
    E, Hd = vc.embed_dim, tc.hidden_size
    sh = {V_PREFIX + "patch_embed.proj.weight": (E, vc.in_channels, vc.temporal_patch_size, vc.patch_size, vc.patch_size)}
    M = E * vc.spatial_merge_size ** 2
    m = V_PREFIX + "merger."
    if vc.arch == "qwen2_5":
        # Qwen2_5_VLVisionBlock: RMSNorm (no bias), SwiGLU MLP with biases; merger ln_q is an RMSNorm
        I = vc.mlp_hidden
        for b in range(vc.depth):
            p = f"{V_PREFIX}blocks.{b}."
            sh.update({p + "norm1.weight": (E,), p + "norm2.weight": (E,),
                       p + "attn.qkv.weight": (3 * E, E), p + "attn.qkv.bias": (3 * E,),
                       p + "attn.proj.weight": (E, E), p + "attn.proj.bias": (E,),
                       p + "mlp.gate_proj.weight": (I, E), p + "mlp.gate_proj.bias": (I,),
                       p + "mlp.up_proj.weight": (I, E), p + "mlp.up_proj.bias": (I,),
                       p + "mlp.down_proj.weight": (E, I), p + "mlp.down_proj.bias": (E,)})
        sh.update({m + "ln_q.weight": (E,), m + "mlp.0.weight": (M, M), m + "mlp.0.bias": (M,),
                   m + "mlp.2.weight": (Hd, M), m + "mlp.2.bias": (Hd,)})
    else:
        for b in range(vc.depth):
            p = f"{V_PREFIX}blocks.{b}."
            sh.update({p + "norm1.weight": (E,), p + "norm1.bias": (E,), p + "norm2.weight": (E,), p + "norm2.bias": (E,),
                       p + "attn.qkv.weight": (3 * E, E), p + "attn.qkv.bias": (3 * E,),
                       p + "attn.proj.weight": (E, E), p + "attn.proj.bias": (E,),
                       p + "mlp.fc1.weight": (vc.mlp_hidden, E), p + "mlp.fc1.bias": (vc.mlp_hidden,),
                       p + "mlp.fc2.weight": (E, vc.mlp_hidden), p + "mlp.fc2.bias": (E,)})
        sh.update({m + "ln_q.weight": (E,), m + "ln_q.bias": (E,), m + "mlp.0.weight": (M, M), m + "mlp.0.bias": (M,),
                   m + "mlp.2.weight": (Hd, M), m + "mlp.2.bias": (Hd,)})
    sh[L_PREFIX + "embed_tokens.weight"] = (tc.vocab_size, Hd)
    qd, kd = tc.num_heads * tc.head_dim, tc.num_kv_heads * tc.head_dim
    for i in range(tc.num_layers):
        p = f"{L_PREFIX}layers.{i}."
        sh.update({p + "input_layernorm.weight": (Hd,), p + "post_attention_layernorm.weight": (Hd,),
                   p + "self_attn.q_proj.weight": (qd, Hd), p + "self_attn.q_proj.bias": (qd,),
                   p + "self_attn.k_proj.weight": (kd, Hd), p + "self_attn.k_proj.bias": (kd,),
                   p + "self_attn.v_proj.weight": (kd, Hd), p + "self_attn.v_proj.bias": (kd,),
                   p + "self_attn.o_proj.weight": (Hd, qd),
                   p + "mlp.gate_proj.weight": (tc.intermediate_size, Hd), p + "mlp.up_proj.weight": (tc.intermediate_size, Hd),
                   p + "mlp.down_proj.weight": (Hd, tc.intermediate_size)})
    sh[L_PREFIX + "norm.weight"] = (Hd,)
    if not tc.tie_word_embeddings:
        sh["lm_head.weight"] = (tc.vocab_size, Hd)
    return sh


def random_state_dict(cfg: ModelConfig, seed: int = 0, device="cpu", dtype=torch.bfloat16, std: float = 0.02):
    """Random-init weights of the real shapes (no checkpoint is available offline): matrices and
    biases N(0, std), norm gains 1 + N(0, std)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    sd = {}
    for name, shape in state_dict_shapes(cfg).items():
        t = torch.randn(shape, generator=g, device=device, dtype=torch.float32) * std
        if name.endswith("norm.weight") or "norm1.weight" in name or "norm2.weight" in name or name.endswith("ln_q.weight") \
                or name.endswith("layernorm.weight"):
            t = t + 1.0
        sd[name] = t.to(dtype)
    return sd


def decisive_state_dict(cfg: ModelConfig, seed: int = 0, device="cpu", dtype=torch.bfloat16, offset: int = 45,
                        gain: float = 20.0, sharpness: float = 4.0):
    """Random weights of the real shapes whose GREEDY TOKEN is decided by a wide margin (tens of times the bf16 noise of a
    28-layer forward) while still depending on the cached context: `random_state_dict` plus one planted attention head.

    With iid random weights the top two of ~152k logits are closer than the rounding noise in a fixed fraction of the
    steps whatever the kernels do, so "token ids exact under greedy" cannot be asserted on them.  The planted head makes
    the network digital the way a trained copy/induction head is:
      * layer 0, kv head 0 and its query heads: q and k come from their BIASES only (weights zeroed) and carry one
        amplitude on the 16 temporal M-RoPE frequency pairs, phased so that after the rotation q(p) . k(p') peaks at
        p - p' == `offset` (`sharpness` = score gap per unit of sum(cos): 1.35 units to the neighbours, > 4.6 beyond);
      * its value / output projections are gamma * P^T P with one random P (128 x hidden): the head writes a copy of the
        (layer-0, i.e. exact) embedding of the token `offset` positions back into the residual stream with RMS `gain`;
      * the tied lm_head reads that copy back as the same token (the 7B's separate lm_head is set equal to the embedding);
      * the chat-template markers the span finder keys on (<|im_start|>, <|im_end|>, <|endoftext|>, the vision markers, "Time")
        are embedded as HALF the embedding of an ordinary stand-in token, so a copied marker decodes to its stand-in and
        the generated text never contains one.
    Every other weight, the whole ViT included, stays N(0, 0.02) and runs at its usual magnitudes; which token comes out
    depends on the KV row `offset` positions back, its slot mapping and its re-indexed position."""
    from .config import ENDOFTEXT, IM_END, IM_START, VIDEO_PAD, VISION_END, VISION_START
    tc = cfg.text
    sd = random_state_dict(cfg, seed, device, dtype)
    g = torch.Generator(device=device)
    g.manual_seed(seed + 7919)
    D, H, G = tc.head_dim, tc.hidden_size, tc.num_heads // tc.num_kv_heads
    n_t = tc.mrope_section[0]                                   # temporal frequency pairs: text tokens' 1-D positions
    inv = 1.0 / (tc.rope_theta ** (torch.arange(0, D, 2, dtype=torch.float64) / D))
    amp = (sharpness * (D ** 0.5)) ** 0.5                       # b^2 * sum(cos) / sqrt(D) = sharpness * sum(cos)
    kb = torch.zeros(D, dtype=torch.float64)
    qb = torch.zeros(D, dtype=torch.float64)
    kb[:n_t] = amp
    qb[:n_t] = amp * torch.cos(inv[:n_t] * offset)
    qb[D // 2:D // 2 + n_t] = -amp * torch.sin(inv[:n_t] * offset)
    p = f"{L_PREFIX}layers.0.self_attn."
    sd[p + "q_proj.weight"][:G * D] = 0
    sd[p + "k_proj.weight"][:D] = 0
    sd[p + "q_proj.bias"][:G * D] = qb.float().repeat(G).to(device=device, dtype=dtype)
    sd[p + "k_proj.bias"][:D] = kb.float().to(device=device, dtype=dtype)
    P = torch.randn((D, H), generator=g, device=device, dtype=torch.float32) * 0.02
    sd[p + "v_proj.weight"][:D] = P.to(dtype)
    sd[p + "v_proj.bias"][:D] = 0
    # |P^T P x| for a unit-RMS x: sigma^2 * sqrt(D^2 + D*H) per coordinate
    gamma = gain / (0.02 ** 2 * (D * D + D * H) ** 0.5)
    sd[p + "o_proj.weight"][:, :G * D] = ((gamma / G) * P.t().repeat(1, G)).to(dtype)
    emb = sd[L_PREFIX + "embed_tokens.weight"]
    for k, s in enumerate((ENDOFTEXT, IM_START, IM_END, VISION_START, VISION_END, VIDEO_PAD, 1462)):      # 1462 = "Time", a span marker
        emb[s] = (0.5 * emb[1000 + 37 * k].float()).to(dtype)
    if not tc.tie_word_embeddings:
        sd["lm_head.weight"] = emb.clone()
    return sd


LLM_FP8_MATRICES = ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                    "mlp.down_proj")


def quantize_rows_fp8_pow2(w: torch.Tensor):
    """Per output row n: s_n = 2^ceil(log2(amax_n / 448)) (exactly: frexp of amax_n / 448 in fp64, whose 53 bits cannot round a
    value above a power of two onto it), zero rows s_n = 1; q = rne_e4m3(w / s_n), which never saturates since |w / s_n| <= 448.
    Returns (q float8_e4m3fn [N, K], s float32 [N]).  W' = q * s_n is exactly representable in bf16, so a GEMV that applies s_n
    once to sum_k q_k x_k computes the bf16 GEMV on W' up to the fp32 summation order."""
    wf = w.detach().float()
    amax = wf.abs().amax(dim=1)
    m, e = torch.frexp(amax.double() / 448.0)                # amax / 448 = m * 2^e, m in [0.5, 1)
    e = torch.where(m == 0.5, e - 1, e)                      # already a power of two: that value
    e = e.clamp(min=-126)                                    # (a scale never needs to be subnormal: the row only gets smaller)
    s = torch.where(amax > 0, torch.pow(2.0, e.double()).float(), torch.ones_like(amax))      # (2^e exact in fp64 and fp32)
    q = (wf / s.unsqueeze(1)).to(torch.float8_e4m3fn)
    return q, s.contiguous()


def dequantize_rows_fp8(q: torch.Tensor, s: torch.Tensor, dtype=torch.bfloat16):
    """W' = q * s_n (exact in bf16)."""
    return (q.float() * s.float().unsqueeze(1)).to(dtype)


def fp8_reference_state_dict(sd: Dict[str, torch.Tensor], cfg: ModelConfig) -> Dict[str, torch.Tensor]:
    """The model an `llm_fp8=True` engine built from `sd` computes, as a bf16 state dict: every LLM layer matrix (q/k/v/o_proj,
    gate/up/down_proj) and the lm_head replaced by W' = dequant(quant(W)).  Biases, norms, the embedding table and the whole vision
    tower stay as they are; with tied embeddings an explicit `lm_head.weight` = W'(embed) is added (the embedding gather keeps
    reading the bf16 table)."""
    tc = cfg.text
    out = dict(sd)
    for i in range(tc.num_layers):
        for m in LLM_FP8_MATRICES:
            k = f"{L_PREFIX}layers.{i}.{m}.weight"
            out[k] = dequantize_rows_fp8(*quantize_rows_fp8_pow2(sd[k]), dtype=sd[k].dtype)
    head = sd[L_PREFIX + "embed_tokens.weight"] if tc.tie_word_embeddings else sd["lm_head.weight"]
    out["lm_head.weight"] = dequantize_rows_fp8(*quantize_rows_fp8_pow2(head), dtype=head.dtype)
    return out


# OCP MX FP4: a nibble is sign + e2m1; the magnitudes of codes 0..7
E2M1_VALUES = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)


def quantize_blocks_mxfp4(w: torch.Tensor):
    """OCP MXFP4 of a [N, K] matrix, K a multiple of 32: per block of 32 consecutive K elements one scale 2^e with e the smallest integer
    such that amax(block) <= 6 * 2^e (taken from the fp32 exponent and mantissa of amax, no division: nothing ever saturates), an
    all-zero block e = 0, e clamped below at -125 (smaller blocks round toward zero and every non-zero W' stays a normal bf16), e > 125
    a ValueError; codes = round-to-nearest-even of w / 2^e onto the e2m1 grid (0, 0.5, 1, 1.5, 2, 3, 4, 6; a tie goes to the even code),
    a zero always +0.  Returns (codes uint8 [N, K / 2], scales uint8 [N, K / 32]): element 2i of a row is the low nibble of byte i,
    element 2i + 1 the high one; scale byte = e + 127 (e8m0; 0xFF is never produced).  W' = code * 2^e is exactly representable in bf16."""
    if w.dim() != 2 or w.shape[1] % 32:
        raise ValueError(f"quantize_blocks_mxfp4: needs a [N, K] matrix with K a multiple of 32 (one block = 32 elements), got {tuple(w.shape)}")
    N, K = w.shape
    wf = w.detach().float().view(N, K // 32, 32)
    amax = wf.abs().amax(dim=2)
    if not bool(torch.isfinite(amax).all()):
        raise ValueError("quantize_blocks_mxfp4: non-finite weights")
    m, ex = torch.frexp(amax)                                # amax = m * 2^ex, m in [0.5, 1); 6 * 2^e = 0.75 * 2^(e + 3)
    e = torch.where(m <= 0.75, ex - 3, ex - 2)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    if int(e.max()) > 125:
        raise ValueError("quantize_blocks_mxfp4: a block needs a scale above 2^125")
    e = e.clamp(min=-125)
    a = torch.ldexp(wf.abs(), -e.unsqueeze(2))               # |w| / 2^e <= 6, exact (a power-of-two factor)
    # the grid's step is 0.5 below 2, 1 up to 4, 2 up to 6; torch.round is half-to-even and an even multiple of the step is an even code
    q = torch.where(a < 2, torch.round(a * 2) / 2, torch.where(a < 4, torch.round(a), torch.round(a / 2) * 2))
    code = torch.where(q <= 2, q * 2, torch.where(q <= 4, q + 2, torch.full_like(q, 7.0))).to(torch.uint8)
    code = torch.where((wf < 0) & (q > 0), code | 8, code).view(N, K)
    codes = (code[:, 0::2] | (code[:, 1::2] << 4)).contiguous()
    return codes, (e + 127).to(torch.uint8).contiguous()


def dequantize_blocks_mxfp4(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16):
    """W' = e2m1(code) * 2^(scale - 127), [N, K] from codes [N, K / 2] and scales [N, K / 32] (exact in bf16)."""
    N, K = codes.shape[0], codes.shape[1] * 2
    lut = torch.tensor(E2M1_VALUES + tuple(-v for v in E2M1_VALUES), dtype=torch.float32, device=codes.device)
    vals = torch.stack([lut[(codes & 0xF).long()], lut[(codes >> 4).long()]], dim=-1).view(N, K // 32, 32)
    return torch.ldexp(vals, (scales.to(torch.int32) - 127).unsqueeze(2)).view(N, K).to(dtype)


def quantize_blocks_mxfp8(x: torch.Tensor):
    """OCP MXFP8 (e4m3 elements) of a bf16 [M, K] activation matrix, K a multiple of 32: per block of 32 consecutive K elements one scale
    2^e with e the smallest integer such that amax(block) <= 448 * 2^e (from the exponent and mantissa of amax, no division: with
    amax = m * 2^ex, m in [0.5, 1), e = ex - 9 if m <= 0.875 else ex - 8; nothing ever saturates), an all-zero block e = 0, e clamped
    below at -117 (quieter blocks round toward zero and every non-zero A' stays a normal bf16; bf16 inputs cannot overflow e8m0 above);
    codes = round-to-nearest-even of x / 2^e (exact: a power of two on an 8-bit significand) onto e4m3 in the `fn` encoding
    (torch.float8_e4m3fn), the sign kept (a -0 or a negative value that rounds to zero is 0x80).  A block that holds an inf or a NaN is
    code 0x7F (NaN) in every element with scale byte 127.  Returns (codes uint8 [M, K], scales uint8 [M, K / 32]), scale byte = e + 127.
    A' = e4m3(code) * 2^e is exactly representable in bf16."""
    if x.dim() != 2 or x.shape[1] % 32:
        raise ValueError(f"quantize_blocks_mxfp8: needs a [M, K] matrix with K a multiple of 32 (one block = 32 elements), got {tuple(x.shape)}")
    if x.dtype != torch.bfloat16:
        raise ValueError(f"quantize_blocks_mxfp8: needs bf16 activations, got {x.dtype}")
    M, K = x.shape
    xf = x.detach().float().view(M, K // 32, 32)
    amax = xf.abs().amax(dim=2)                              # (a NaN propagates)
    bad = ~torch.isfinite(amax)
    amax = torch.where(bad, torch.zeros_like(amax), amax)
    xf = torch.where(bad.unsqueeze(2), torch.zeros_like(xf), xf)
    m, ex = torch.frexp(amax)                                # amax = m * 2^ex, m in [0.5, 1); 448 * 2^e = 0.875 * 2^(e + 9)
    e = torch.where(m <= 0.875, ex - 9, ex - 8)
    e = torch.where(amax > 0, e, torch.zeros_like(e)).clamp(min=-117)
    a = torch.ldexp(xf.double(), -e.unsqueeze(2)).float()    # x / 2^e, |.| <= 448, exact (fp64 keeps 2^-e and the product normal)
    codes = a.to(torch.float8_e4m3fn).view(torch.uint8)
    codes = torch.where(bad.unsqueeze(2), torch.full_like(codes, 0x7F), codes).view(M, K).contiguous()
    scales = torch.where(bad, torch.full_like(e, 127), e + 127).to(torch.uint8).contiguous()
    return codes, scales


def dequantize_blocks_mxfp8(codes: torch.Tensor, scales: torch.Tensor, dtype=torch.bfloat16):
    """A' = e4m3(code) * 2^(scale - 127), [M, K] from codes [M, K] and scales [M, K / 32] (exact in bf16; a NaN code stays NaN)."""
    M, K = codes.shape
    vals = codes.contiguous().view(torch.float8_e4m3fn).float().view(M, K // 32, 32)
    return torch.ldexp(vals.double(), (scales.to(torch.int32) - 127).unsqueeze(2)).view(M, K).to(dtype)


def fp4_reference_state_dict(sd: Dict[str, torch.Tensor], cfg: ModelConfig) -> Dict[str, torch.Tensor]:
    """The model an `llm_fp4=True` engine built from `sd` computes, as a bf16 state dict: every LLM layer matrix (q/k/v/o_proj,
    gate/up/down_proj) replaced by its MXFP4 W' = dequant(quant(W)), the lm_head by its e4m3 W' exactly as `fp8_reference_state_dict`
    does it (the head of an fp4 engine stays e4m3).  Everything else stays as it is."""
    tc = cfg.text
    out = dict(sd)
    for i in range(tc.num_layers):
        for m in LLM_FP8_MATRICES:
            k = f"{L_PREFIX}layers.{i}.{m}.weight"
            out[k] = dequantize_blocks_mxfp4(*quantize_blocks_mxfp4(sd[k]), dtype=sd[k].dtype)
    head = sd[L_PREFIX + "embed_tokens.weight"] if tc.tie_word_embeddings else sd["lm_head.weight"]
    out["lm_head.weight"] = dequantize_rows_fp8(*quantize_rows_fp8_pow2(head), dtype=head.dtype)
    return out


class EngineWeights:
    """Fused, contiguous, device-resident views the kernels consume.

    `llm_fp8`: the LLM layer matrices and the lm_head are kept as e4m3 with one power-of-two scale per row (quantize_rows_fp8_pow2),
    quantised layer by layer so that no bf16 copy of all layers ever exists; per layer `flat8` (qkv | o | gate/up | down, back to
    back) and `scale` (their rows' scales, same order) with the views `<name>8` / `<name>_s`; `lm_head8` / `lm_head_s`.  The bf16
    embedding table stays.

    `llm_fp4`: the layer matrices are kept as OCP MXFP4 (quantize_blocks_mxfp4), again one matrix at a time; per layer `flat4` (the codes
    of qkv | o | gate/up | down, back to back) and `scale4` (their block scales, same order) with the views `<name>4` [N, K / 2] and
    `<name>_s4` [N, K / 32]; the lm_head is e4m3 as with `llm_fp8` (`lm_head8` / `lm_head_s`)."""

    def __init__(self, sd: Dict[str, torch.Tensor], cfg: ModelConfig, device, llm_fp8: bool = False, llm_fp4: bool = False):
        vc, tc = cfg.vision, cfg.text
        want = state_dict_shapes(cfg)
        missing = [k for k in want if k not in sd]
        if missing:
            raise KeyError(f"state dict lacks {len(missing)} tensors, e.g. {missing[:3]}")
        for k, shp in want.items():
            if tuple(sd[k].shape) != tuple(shp):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != expected {shp}")

        def dev(t):
            return t.detach().to(device=device, dtype=torch.bfloat16).contiguous()

        self.patch_embed = dev(sd[V_PREFIX + "patch_embed.proj.weight"].reshape(vc.embed_dim, -1))
        self.vit = []
        m = V_PREFIX + "merger."
        if vc.arch == "qwen2_5":
            I, Ip, E = vc.mlp_hidden, vc.mlp_padded, vc.embed_dim
            for b in range(vc.depth):
                p = f"{V_PREFIX}blocks.{b}."
                blk = {k: dev(sd[p + n]) for k, n in [
                    ("n1w", "norm1.weight"), ("n2w", "norm2.weight"), ("qkv_w", "attn.qkv.weight"), ("qkv_b", "attn.qkv.bias"),
                    ("proj_w", "attn.proj.weight"), ("proj_b", "attn.proj.bias"), ("down_b", "mlp.down_proj.bias")]}
                # gate and up fused row-wise, each padded with zero rows to a multiple of 8 (3420 -> 3424): the pad columns of
                # h = silu(0) * 0 are exactly 0 and meet zero columns of down_proj, so the result is unchanged bit for bit
                gu_w = torch.zeros((2 * Ip, E), dtype=torch.bfloat16, device=device)
                gu_b = torch.zeros(2 * Ip, dtype=torch.bfloat16, device=device)
                gu_w[:I].copy_(sd[p + "mlp.gate_proj.weight"]); gu_w[Ip:Ip + I].copy_(sd[p + "mlp.up_proj.weight"])
                gu_b[:I].copy_(sd[p + "mlp.gate_proj.bias"]); gu_b[Ip:Ip + I].copy_(sd[p + "mlp.up_proj.bias"])
                down_w = torch.zeros((E, Ip), dtype=torch.bfloat16, device=device)
                down_w[:, :I].copy_(sd[p + "mlp.down_proj.weight"])
                blk.update(gu_w=gu_w, gu_b=gu_b, down_w=down_w)
                self.vit.append(blk)
            self.merger = {k: dev(sd[m + n]) for k, n in [("ln_w", "ln_q.weight"), ("w0", "mlp.0.weight"), ("b0", "mlp.0.bias"),
                                                           ("w2", "mlp.2.weight"), ("b2", "mlp.2.bias")]}
        else:
            for b in range(vc.depth):
                p = f"{V_PREFIX}blocks.{b}."
                self.vit.append({k: dev(sd[p + n]) for k, n in [
                    ("n1w", "norm1.weight"), ("n1b", "norm1.bias"), ("n2w", "norm2.weight"), ("n2b", "norm2.bias"),
                    ("qkv_w", "attn.qkv.weight"), ("qkv_b", "attn.qkv.bias"), ("proj_w", "attn.proj.weight"),
                    ("proj_b", "attn.proj.bias"), ("fc1_w", "mlp.fc1.weight"), ("fc1_b", "mlp.fc1.bias"),
                    ("fc2_w", "mlp.fc2.weight"), ("fc2_b", "mlp.fc2.bias")]})
            self.merger = {k: dev(sd[m + n]) for k, n in [("ln_w", "ln_q.weight"), ("ln_b", "ln_q.bias"), ("w0", "mlp.0.weight"),
                                                           ("b0", "mlp.0.bias"), ("w2", "mlp.2.weight"), ("b2", "mlp.2.bias")]}
        self.embed = dev(sd[L_PREFIX + "embed_tokens.weight"])
        self.llm_fp8, self.llm_fp4 = bool(llm_fp8), bool(llm_fp4)
        if self.llm_fp8 and self.llm_fp4:
            raise ValueError("llm_fp8 and llm_fp4 are two formats of the same matrices: choose one")
        if self.llm_fp8 or self.llm_fp4:
            need, why = (32, "one MX block = 32 weights") if self.llm_fp4 else (16, "one 16-B load = 16 weights")
            for name, K in (("hidden", tc.hidden_size), ("q width", tc.num_heads * tc.head_dim), ("intermediate", tc.intermediate_size)):
                if K % need:
                    raise ValueError(f"{'llm_fp4' if self.llm_fp4 else 'llm_fp8'} needs K a multiple of {need} ({why}): {name} is {K}")
            self.lm_head = None
            self.lm_head8, self.lm_head_s = quantize_rows_fp8_pow2(
                (self.embed if tc.tie_word_embeddings else sd["lm_head.weight"]).to(device=device))
        else:
            self.lm_head = self.embed if tc.tie_word_embeddings else dev(sd["lm_head.weight"])
        self.final_norm = dev(sd[L_PREFIX + "norm.weight"])
        self.layers = []
        for i in range(tc.num_layers):
            p = f"{L_PREFIX}layers.{i}."
            qkv_w = torch.cat([sd[p + "self_attn.q_proj.weight"], sd[p + "self_attn.k_proj.weight"], sd[p + "self_attn.v_proj.weight"]], 0)
            qkv_b = torch.cat([sd[p + "self_attn.q_proj.bias"], sd[p + "self_attn.k_proj.bias"], sd[p + "self_attn.v_proj.bias"]], 0)
            gu_w = torch.cat([sd[p + "mlp.gate_proj.weight"], sd[p + "mlp.up_proj.weight"]], 0)
            # the four matrices of a layer live back to back in ONE buffer (streamed in this order by a decode step),
            # so the next layer can be pulled into the Infinity Cache with a single range prefetch
            mats = [("qkv_w", qkv_w), ("o_w", sd[p + "self_attn.o_proj.weight"]), ("gu_w", gu_w), ("down_w", sd[p + "mlp.down_proj.weight"])]
            if self.llm_fp8:
                self.layers.append(self._fp8_layer(sd, p, qkv_b, mats, device, dev))
                continue
            if self.llm_fp4:
                self.layers.append(self._fp4_layer(sd, p, qkv_b, mats, device, dev))
                continue
            flat = torch.empty(sum(m.numel() for _, m in mats), dtype=torch.bfloat16, device=device)
            layer = dict(ln1=dev(sd[p + "input_layernorm.weight"]), ln2=dev(sd[p + "post_attention_layernorm.weight"]), qkv_b=dev(qkv_b), flat=flat)
            off = 0
            for name, m in mats:
                view = flat[off:off + m.numel()].view(m.shape)
                view.copy_(m)
                layer[name] = view
                off += m.numel()
            self.layers.append(layer)

    @staticmethod
    def _fp8_layer(sd, p, qkv_b, mats, device, dev):
        """One layer in e4m3: each matrix is quantised on `device` on its own, so at most one bf16 matrix exists beside the fp8 ones."""
        rows = sum(m.shape[0] for _, m in mats)
        flat8 = torch.empty(sum(m.numel() for _, m in mats), dtype=torch.float8_e4m3fn, device=device)
        scale = torch.empty(rows, dtype=torch.float32, device=device)
        layer = dict(ln1=dev(sd[p + "input_layernorm.weight"]), ln2=dev(sd[p + "post_attention_layernorm.weight"]), qkv_b=dev(qkv_b),
                     flat8=flat8, scale=scale)
        off = r0 = 0
        for name, m in mats:
            q, s8 = quantize_rows_fp8_pow2(m.to(device=device))
            view = flat8[off:off + m.numel()].view(m.shape)
            view.copy_(q)
            scale[r0:r0 + m.shape[0]].copy_(s8)
            layer[name + "8"] = view
            layer[name + "_s"] = scale[r0:r0 + m.shape[0]]
            del q, s8
            off += m.numel()
            r0 += m.shape[0]
        return layer

    @staticmethod
    def _fp4_layer(sd, p, qkv_b, mats, device, dev):
        """One layer in MXFP4: each matrix is quantised on `device` on its own, so at most one bf16 matrix exists beside the fp4 ones."""
        n_w = sum(m.numel() for _, m in mats)
        flat4 = torch.empty(n_w // 2, dtype=torch.uint8, device=device)
        scale4 = torch.empty(n_w // 32, dtype=torch.uint8, device=device)
        layer = dict(ln1=dev(sd[p + "input_layernorm.weight"]), ln2=dev(sd[p + "post_attention_layernorm.weight"]), qkv_b=dev(qkv_b),
                     flat4=flat4, scale4=scale4)
        off = 0
        for name, m in mats:
            codes, sc = quantize_blocks_mxfp4(m.to(device=device))
            N, K = m.shape
            layer[name + "4"] = flat4[off // 2:(off + N * K) // 2].view(N, K // 2)
            layer[name + "_s4"] = scale4[off // 32:(off + N * K) // 32].view(N, K // 32)
            layer[name + "4"].copy_(codes)
            layer[name + "_s4"].copy_(sc)
            del codes, sc
            off += N * K
        return layer

    def decode_bytes(self) -> int:
        """Weight bytes one decode step streams (layers + final norm + lm_head): e4m3 codes and their row scales with `llm_fp8`, e2m1
        codes and their block scales (and the e4m3 head) with `llm_fp4`."""
        n = self.final_norm.numel() * 2
        if self.llm_fp8 or self.llm_fp4:
            n += self.lm_head8.numel() + self.lm_head_s.numel() * 4
        else:
            n += self.lm_head.numel() * 2
        for l in self.layers:
            n += sum(t.numel() * t.element_size() for k, t in l.items() if k not in ("flat", "flat8", "scale", "flat4", "scale4"))
        return n

    def decode_weight_bytes(self) -> int:
        return self.decode_bytes()

    def nbytes_llm_decode(self) -> int:
        return self.decode_bytes()
