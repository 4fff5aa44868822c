"""Fused NHWC BatchNorm(+residual+ReLU) — python surface.

The hot elementwise chain of the ResNet benchmark:
    bn -> (+ residual) -> relu          (forward)
    relu-mask -> bn-bwd -> dres         (backward)
runs as hand-written gfx950 kernels (csrc/bn_ops.hip): bf16-native (no
autocast fp32 round-trip), residual-add and ReLU folded into the normalize /
gradient passes. On CPU (CI) the same math runs through torch's own
batch-norm kernels, so numerics tests can compare and a fused=True model
equals its unfused twin bit for bit there.

`FusedBatchNorm2d` is state_dict-compatible with nn.BatchNorm2d (same
parameter/buffer names).
"""
from typing import Optional

import torch

from autodist_amd.ops import api as ops_api


class _FusedBNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, relu, residual, ws=None):
        use_hip = x.is_cuda and ops_api.has_gpu_ops()
        ctx.ws_bwd = ws[1] if ws is not None else None
        if use_hip and relu:
            # backward needs y only for its sign: the apply kernel packs
            # y > 0 into one bit per element, and that mask is saved instead
            y, save_mean, save_rstd, sign = ops_api.ext().bn_fwd_train_mask(
                x, weight, bias, running_mean, running_var, residual,
                eps, momentum, relu, ws[0] if ws is not None else None)
        elif use_hip:
            y, save_mean, save_rstd = ops_api.ext().bn_fwd_train(
                x, weight, bias, running_mean, running_var, residual,
                eps, momentum, relu, ws[0] if ws is not None else None)
            sign = y  # not read when relu is off
        else:
            # torch's own batch-norm kernels, so that a fused=True model is
            # the unfused model on this path down to the last bit, however
            # ill-conditioned the network (tests/test_fused_bn.py)
            xf = x.float()
            m = xf.numel() // xf.size(1)
            with torch.no_grad():
                if m > 1:
                    y, save_mean, save_rstd = torch.native_batch_norm(
                        xf, weight, bias, running_mean, running_var, True,
                        momentum, eps)
                else:
                    # one value per channel: var = 0, and the unbiased
                    # estimate is taken as 0 too, not 0/0
                    y, save_mean, save_rstd = torch.native_batch_norm(
                        xf, weight, bias, None, None, True, momentum, eps)
                    running_mean.mul_(1 - momentum).add_(save_mean,
                                                         alpha=momentum)
                    running_var.mul_(1 - momentum)
                if residual is not None:
                    y = y + residual.float()
                if relu:
                    y = torch.relu(y)
                y = y.to(x.dtype)
            sign = y
        ctx.save_for_backward(x, sign, save_mean, save_rstd, weight)
        ctx.relu = relu
        ctx.has_res = residual is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        # sign: y itself, or on the HIP path with relu its packed y > 0 mask
        x, sign, save_mean, save_rstd, weight = ctx.saved_tensors
        relu, has_res = ctx.relu, ctx.has_res
        use_hip = x.is_cuda and ops_api.has_gpu_ops()
        if use_hip:
            bwd = ops_api.ext().bn_bwd_mask if relu else ops_api.ext().bn_bwd
            out = bwd(x, dy.contiguous(
                memory_format=torch.channels_last), sign, save_mean, save_rstd,
                weight, relu, has_res, ctx.ws_bwd)
            dx, dweight, dbias = out[0], out[1], out[2]
            dres = out[3] if has_res else None
        else:
            dyf = dy.float()
            if relu:
                dyf = dyf * (sign > 0).float()
            dres = dyf.to(dy.dtype) if has_res else None
            dxf, dweight, dbias = torch.ops.aten.native_batch_norm_backward(
                dyf, x.float(), weight, None, None, save_mean, save_rstd,
                True, 0.0, [True, True, True])
            dx = dxf.to(x.dtype)
        return (dx, dweight, dbias, None, None, None, None, None, dres, None)


def fused_bn_train(x, weight, bias, running_mean, running_var,
                   momentum=0.1, eps=1e-5, relu=False,
                   residual: Optional[torch.Tensor] = None, ws=None):
    return _FusedBNFunction.apply(x, weight, bias, running_mean, running_var,
                                  momentum, eps, relu, residual, ws)


class FusedBatchNorm2d(torch.nn.Module):
    """Drop-in BatchNorm2d with optional fused ReLU and residual add.

    forward(x) applies bn [+relu]; forward_add(x, residual) applies
    bn(x) + residual -> relu (the Bottleneck tail).
    """

    def __init__(self, num_features, eps=1e-5, momentum=0.1, relu=False):
        super().__init__()
        self.num_features = num_features
        self.eps = eps
        self.momentum = momentum
        self.relu = relu
        self.weight = torch.nn.Parameter(torch.ones(num_features))
        self.bias = torch.nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_mean", torch.zeros(num_features))
        self.register_buffer("running_var", torch.ones(num_features))
        self.register_buffer("num_batches_tracked",
                             torch.tensor(0, dtype=torch.long))
        self._ws = None  # persistent kernel workspaces (not in state_dict)

    def _check(self, x):
        if x.is_cuda and not x.is_contiguous(memory_format=torch.channels_last):
            x = x.contiguous(memory_format=torch.channels_last)
        return x

    def forward(self, x, residual: Optional[torch.Tensor] = None):
        x = self._check(x)
        if residual is not None:
            residual = self._check(residual)
        if self.training:
            self.num_batches_tracked += 1
            if x.is_cuda and (self._ws is None
                              or self._ws[0].device != x.device):
                # layouts match BN_GM_MAX=512 in csrc/ext.hip: reduce
                # partials plus scale/shift (fwd) and k1..k3 (bwd). Only
                # values that are dead when the call returns live here;
                # save_mean/save_rstd come back freshly allocated, so calling
                # this module twice before backward is safe.
                self._ws = (
                    torch.empty(2 * 512 + 4, self.num_features,
                                device=x.device),
                    torch.empty(2 * 512 + 3, self.num_features,
                                device=x.device))
            return fused_bn_train(x, self.weight, self.bias,
                                  self.running_mean, self.running_var,
                                  self.momentum, self.eps, self.relu, residual,
                                  ws=self._ws if x.is_cuda else None)
        # eval: running-stat normalize (+add+relu)
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        shift = self.bias - self.running_mean * scale
        y = x * scale[None, :, None, None].to(x.dtype) + \
            shift[None, :, None, None].to(x.dtype)
        if residual is not None:
            y = y + residual
        return torch.relu(y) if self.relu else y

    def forward_add(self, x, residual):
        return self.forward(x, residual)

    def extra_repr(self):
        return f"{self.num_features}, relu={self.relu}"
