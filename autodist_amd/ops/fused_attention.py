"""Fused MFMA attention (gfx950) — forward + backward, mask + dropout.

`fused_sdpa(q, k, v, ...)` runs the hand-written CDNA4 MFMA attention
kernels (ops/csrc/attention.hip 4-wave LDS-tiled forward;
attention_bwd.hip FA2-style backward, GPU-validated vs fp32 autograd) when
applicable, else falls back to torch SDPA. Applicability: q, k, v bf16 of
one shape [B, H, S, D], head_dim 64 or 128, S % 32 == 0, mask absent or a
key-padding mask broadcastable to [B, 1, 1, S], any dropout_p < 1 — the
BERT/transformer hot path for both serving and training. Dropout uses a
counter-based hash of (seed, bh, q, k) regenerated identically in the
backward (flash-attention style, no S x S state); the seed is drawn
host-side per forward call.
"""
import math
import random
from typing import Optional

import torch

from autodist_amd.ops import api as ops_api


def _mask_rows(attn_mask, q) -> Optional[torch.Tensor]:
    """The [B | 1, S] rows of a supported key-padding mask, else None.
    Supported, and the ONLY forms can_use_fused accepts: on q's device,
    [B, 1, 1, S], its batch-broadcast form [1, 1, 1, S], or the 2-D
    [B, S]."""
    B, S = q.size(0), q.size(-2)
    m = attn_mask
    if m.device != q.device:
        return None
    if m.dim() == 4 and m.size(1) == 1 and m.size(2) == 1:
        m = m[:, 0, 0, :]
        if m.size(1) == S and m.size(0) in (1, B):
            return m
        return None
    if m.dim() == 2 and m.shape == (B, S):
        return m
    return None


def _key_padding_mask(attn_mask, q) -> Optional[torch.Tensor]:
    """Convert a supported mask to the kernels' additive fp32 [B, S] form
    (a batch-broadcast mask is expanded: the kernels index it by batch).
    Returns None when no mask, raises ValueError when unsupported."""
    if attn_mask is None:
        return None
    B, S = q.size(0), q.size(-2)
    m = _mask_rows(attn_mask, q)
    if m is None:
        raise ValueError("not a key-padding mask")
    if m.dtype == torch.bool:
        # True = attend (torch SDPA convention) -> additive 0 / -30000
        m = torch.zeros(m.shape, dtype=torch.float32,
                        device=m.device).masked_fill_(~m, -30000.0)
    return m.to(torch.float32).expand(B, S).contiguous()


def can_use_fused(q, attn_mask, dropout_p, k=None, v=None) -> bool:
    """Kernel applicability (training AND inference; reference context: the
    reference leaves attention to TF ops — hand-written CDNA4 here is the
    north-star requirement). k / v, when given, must match q in shape,
    dtype and device (self-attention): cross-attention lengths, another
    head dim or dtype go to torch SDPA. Accepts exactly the masks
    _key_padding_mask converts."""
    if not (q.dim() == 4 and q.is_cuda and q.dtype == torch.bfloat16
            and q.size(-1) in (64, 128)
            and q.size(-2) % 32 == 0 and q.size(-2) >= 32
            and 0.0 <= dropout_p < 1.0 and ops_api.has_gpu_ops()):
        return False
    for t in (k, v):
        if t is not None and not (t.shape == q.shape and t.dtype == q.dtype
                                  and t.device == q.device):
            return False
    if attn_mask is None:
        return True
    return _mask_rows(attn_mask, q) is not None


class FusedAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, mask, p_drop, seed):
        o = ops_api.ext().attn_fwd(q, k, v, scale, mask, p_drop, seed)
        ctx.save_for_backward(q, k, v, o, *([mask] if mask is not None
                                            else []))
        ctx.scale = scale
        ctx.p_drop = p_drop
        ctx.seed = seed
        ctx.has_mask = mask is not None
        return o

    @staticmethod
    def backward(ctx, dout):
        if ctx.has_mask:
            q, k, v, o, mask = ctx.saved_tensors
        else:
            (q, k, v, o), mask = ctx.saved_tensors, None
        dq, dk, dv = ops_api.ext().attn_bwd(q, k, v, o, dout.contiguous(),
                                            ctx.scale, mask, ctx.p_drop,
                                            ctx.seed)
        return dq, dk, dv, None, None, None, None


def fused_sdpa(q, k, v, attn_mask: Optional[torch.Tensor] = None,
               dropout_p: float = 0.0, scale: Optional[float] = None):
    """Drop-in for torch SDPA on [B, H, S, D] tensors.

    Note: dropout_p is applied only in training-style calls; callers pass
    0.0 for eval (as the models do). The dropout mask differs from torch's
    RNG but is a valid iid Bernoulli(1-p) mask with exact fwd/bwd
    consistency.
    """
    if scale is None:
        scale = 1.0 / math.sqrt(q.size(-1))
    if can_use_fused(q, attn_mask, dropout_p, k, v):
        mask = _key_padding_mask(attn_mask, q)
        seed = random.getrandbits(31) if dropout_p > 0.0 else 0
        # kernels are stride-aware in B/H/S (head dim must be contiguous):
        # transposed views of the fused qkv projection pass through with
        # ZERO copies
        def _ok(t):
            return t if t.stride(-1) == 1 else t.contiguous()
        return FusedAttentionFn.apply(_ok(q), _ok(k), _ok(v), scale, mask,
                                      float(dropout_p), seed)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=attn_mask, dropout_p=dropout_p, scale=scale)
