"""Fused bf16 LayerNorm (+ residual add) module for transformer streams.

torch's LayerNorm under bf16 autocast upcasts to fp32 and returns fp32,
so every transformer block pays bfloat16<->float32 copy kernels around
each LN and keeps an fp32 residual stream (measured: the cast/elementwise
cluster was ~13% of the BERT-base step). FusedLayerNorm keeps the
residual stream bf16 end to end: one gfx950 kernel reads bf16, folds the
residual add in, normalizes with fp32 row statistics, and writes bf16
(ops/csrc/ln_ops.hip; backward = dx kernel + chunked dgamma/dbeta
partials). Parameter names match nn.LayerNorm (weight/bias) so state
dicts are interchangeable.

forward(x, residual, dropout_p=p) in training mode computes
LayerNorm(dropout_p(x) + residual) in one kernel each way (ln_drop_fwd /
ln_drop_bwd): the dropout mask is the attention kernels' counter hash of
(seed, row, col), regenerated in the backward, so neither a dropped copy nor
a mask is stored. The seed is drawn host-side per call, as in fused_sdpa.
AUTODIST_LN_DROPOUT=torch keeps F.dropout in front of the plain kernels.

Reference context: the reference delegates all normalization math to TF
ops (SURVEY §2.3 — zero native files); hand-written CDNA4 normalization
on the training hot path is the rebuild's north-star requirement, like
the fused BN trio (ops/csrc/bn_ops.hip) for the CNN side.
"""
import os
import random
from typing import Optional

import torch

from autodist_amd.ops import api as ops_api


class _FusedLNFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, res, weight, bias, eps):
        y, u, mean, rstd = ops_api.ext().ln_fwd(x, res, weight, bias, eps)
        ctx.save_for_backward(u, weight, mean, rstd)
        ctx.has_res = res is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        u, weight, mean, rstd = ctx.saved_tensors
        dx, dgamma, dbeta = ops_api.ext().ln_bwd(dy.contiguous(), u, weight,
                                                 mean, rstd)
        # d(x + res)/dx == d(x + res)/dres == identity
        return (dx, dx if ctx.has_res else None, dgamma, dbeta, None)


class _FusedDropLNFn(torch.autograd.Function):
    """y = LN(dropout_p(x) + res); the hash mask of `seed` is regenerated in
    the backward, which returns distinct gradients for x and res."""

    @staticmethod
    def forward(ctx, x, res, weight, bias, eps, p, seed):
        y, u, mean, rstd = ops_api.ext().ln_drop_fwd(x, res, weight, bias,
                                                     eps, p, seed)
        ctx.save_for_backward(u, weight, mean, rstd)
        ctx.has_res = res is not None
        ctx.p, ctx.seed = p, seed
        return y

    @staticmethod
    def backward(ctx, dy):
        u, weight, mean, rstd = ctx.saved_tensors
        dx, dres, dgamma, dbeta = ops_api.ext().ln_drop_bwd(
            dy.contiguous(), u, weight, mean, rstd, ctx.p, ctx.seed)
        return (dx, dres if ctx.has_res else None, dgamma, dbeta, None, None,
                None)


def can_use_ln_dropout_kernels(x, residual, hidden) -> bool:
    """Shapes the ln_drop_* kernels serve: bf16 on the GPU, H % 8 == 0,
    8 <= H <= 4096, 16-byte aligned bases (checked on the contiguous
    tensors the module hands over)."""
    if os.environ.get("AUTODIST_LN_DROPOUT", "") == "torch":
        return False
    if not (x.is_cuda and x.dtype == torch.bfloat16 and hidden % 8 == 0
            and 8 <= hidden <= 4096 and ops_api.has_gpu_ops()):
        return False
    return all(t is None or (t.dtype == torch.bfloat16
                             and t.data_ptr() % 16 == 0)
               for t in (x, residual))


class FusedLayerNorm(torch.nn.Module):
    """Drop-in nn.LayerNorm with optional fused residual:
    forward(x, residual) == LayerNorm(x + residual).

    Under autocast the bf16 path keeps inputs AND outputs bf16 (fp32 row
    stats inside the kernel) — the standard bf16-residual-stream design —
    where torch LN would return fp32. CPU / non-bf16 inputs fall back to
    torch's layer_norm in fp32.

    dropout_p > 0 in training mode drops x before the residual add:
    forward(x, residual, dropout_p=p) == LayerNorm(dropout(x) + residual),
    fused into the kernels where they serve the shape, else F.dropout in
    front of the path above."""

    def __init__(self, hidden: int, eps: float = 1e-12):
        super().__init__()
        self.hidden = hidden
        self.eps = eps
        self.weight = torch.nn.Parameter(torch.ones(hidden))
        self.bias = torch.nn.Parameter(torch.zeros(hidden))

    def forward(self, x, residual: Optional[torch.Tensor] = None,
                dropout_p: float = 0.0):
        if torch.is_autocast_enabled() and x.is_cuda:
            x = x.to(torch.bfloat16)
            if residual is not None:
                residual = residual.to(torch.bfloat16)
        if self.training and dropout_p > 0.0:
            xc = x.contiguous()
            rc = residual.contiguous() if residual is not None else None
            if dropout_p < 1.0 and can_use_ln_dropout_kernels(
                    xc, rc, self.hidden):
                return _FusedDropLNFn.apply(
                    xc, rc, self.weight, self.bias, self.eps,
                    float(dropout_p), random.getrandbits(31))
            x = torch.nn.functional.dropout(x, dropout_p, True)
        if (x.is_cuda and x.dtype == torch.bfloat16
                and self.hidden <= 4096 and self.hidden % 2 == 0
                and ops_api.has_gpu_ops()):
            return _FusedLNFn.apply(
                x.contiguous(),
                residual.contiguous() if residual is not None else None,
                self.weight, self.bias, self.eps)
        t = x if residual is None else x + residual
        return torch.nn.functional.layer_norm(
            t, (self.hidden,), self.weight, self.bias, self.eps)

    def extra_repr(self):
        return f"{self.hidden}, eps={self.eps}, fused_bf16"
