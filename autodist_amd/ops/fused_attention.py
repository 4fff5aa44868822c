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

Without dropout the forward also exists as a split-KV variant
(ops/csrc/attention_split.hip): `kv_splits` workgroups share the keys of one
query block and a combine kernel merges their partial softmaxes. It is chosen
by `fused_sdpa(..., kv_splits=n)`, by AUTODIST_ATTN_KV_SPLITS, or by
`auto_kv_splits` where the one-kernel grid leaves most of the GPU idle.
"""
import math
import os
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


ATTN_MAX_SPLITS = 8    # csrc/attention_split.hip
# Grid-fill level of the dispatch rule, in workgroups per CU: the split path
# is chosen while the one-kernel grid nqb * B * H is below
# SPLIT_FILL * multi_processor_count. Measured on MI355X (profiles/
# ANALYSIS.md, "Split-KV attention forward"): grids of 48, 96 and 128
# workgroups on 256 CUs are faster split, 192 and above are not; D = 128 was
# measured only at a grid that loses, so the rule takes D = 64 alone.
SPLIT_FILL = 0.75


def auto_kv_splits(B, H, S, D, n_cu, fill=None) -> int:
    """Split count the dispatch rule picks for a dropout-free forward, 0 for
    the one-kernel path. Splitting pays an fp32 write and read of
    splits x |O|, so it is chosen only where the grid is the problem:
    S >= 512 (the regime where the one-kernel forward was measured behind)
    and fewer than fill * n_cu workgroups. The count is the smallest that
    reaches that level, capped at ATTN_MAX_SPLITS and at half the 64-key
    tiles (a split keeps at least two tiles, so its double buffer overlaps
    a load with compute)."""
    fill = SPLIT_FILL if fill is None else fill
    if S < 512 or D != 64:
        return 0
    grid = -(-S // 128) * B * H          # RB = 2 from S >= 256
    want = fill * n_cu
    if grid >= want:
        return 0
    n = min(math.ceil(want / grid), ATTN_MAX_SPLITS, -(-S // 64) // 2)
    return n if n >= 2 else 0


def _env_kv_splits() -> int:
    """AUTODIST_ATTN_KV_SPLITS: unset or 0 = dispatch rule, 1 = never split,
    n = force n splits."""
    raw = os.environ.get("AUTODIST_ATTN_KV_SPLITS", "0") or "0"
    n = int(raw)
    if n < 0:
        raise ValueError(f"AUTODIST_ATTN_KV_SPLITS must be >= 0, got {raw}")
    return n


class FusedAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, scale, mask, p_drop, seed, kv_splits=0):
        # kv_splits >= 1: split-KV forward (p_drop == 0 only; the binding
        # refuses anything else). The backward recomputes m and l from q
        # and k and needs only the saved o, so it is the same either way.
        if kv_splits:
            o = ops_api.ext().attn_fwd_split(q, k, v, scale, mask,
                                             kv_splits, p_drop)
        else:
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
        return dq, dk, dv, None, None, None, None, None


def fused_sdpa(q, k, v, attn_mask: Optional[torch.Tensor] = None,
               dropout_p: float = 0.0, scale: Optional[float] = None,
               kv_splits: Optional[int] = None):
    """Drop-in for torch SDPA on [B, H, S, D] tensors.

    kv_splits: an integer >= 1 forces the split-KV forward with that many
    key ranges (1 included: bit-equal to the one-kernel forward); it needs
    dropout_p == 0. None leaves the choice to AUTODIST_ATTN_KV_SPLITS and
    then to `auto_kv_splits`. Ignored where the fused kernels do not apply.

    Note: dropout_p is applied only in training-style calls; callers pass
    0.0 for eval (as the models do). The dropout mask differs from torch's
    RNG but is a valid iid Bernoulli(1-p) mask with exact fwd/bwd
    consistency.
    """
    if kv_splits is not None:
        if kv_splits < 1:
            raise ValueError(f"kv_splits must be >= 1, got {kv_splits}")
        if dropout_p > 0.0:
            raise ValueError("kv_splits needs dropout_p == 0: the split-KV "
                             "forward has no dropout")
    if scale is None:
        scale = 1.0 / math.sqrt(q.size(-1))
    if can_use_fused(q, attn_mask, dropout_p, k, v):
        mask = _key_padding_mask(attn_mask, q)
        splits = 0
        if kv_splits is not None:
            splits = int(kv_splits)
        elif dropout_p == 0.0:
            env = _env_kv_splits()
            if env >= 2:
                splits = env
            elif env == 0:
                splits = auto_kv_splits(
                    *q.shape, torch.cuda.get_device_properties(
                        q.device).multi_processor_count)
        seed = random.getrandbits(31) if dropout_p > 0.0 else 0
        # kernels are stride-aware in B/H/S (head dim must be contiguous):
        # transposed views of the fused qkv projection pass through with
        # ZERO copies
        def _ok(t):
            return t if t.stride(-1) == 1 else t.contiguous()
        return FusedAttentionFn.apply(_ok(q), _ok(k), _ok(v), scale, mask,
                                      float(dropout_p), seed, splits)
    return torch.nn.functional.scaled_dot_product_attention(
        q, k, v, attn_mask=attn_mask, dropout_p=dropout_p, scale=scale)
