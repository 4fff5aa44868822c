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


# True routes forward_pool / forward_add_bn through the separate kernels they
# replace (bn -> F.max_pool2d, bn_ds -> bn.forward_add) and makes the *_pair
# tails return one tensor twice, so that autograd adds the two gradients
# itself: the A/B switch of tools/bn_microbench.py and the reference of the
# GPU tests.
SPLIT_PATH = False


def _two_handles(ctx, y):
    """(y, a view of y): autograd hands backward the gradient of each handle
    on its own instead of their sum, and None for a handle nobody used."""
    ctx.set_materialize_grads(False)
    return y, y.view_as(y)


def _nhwc_grad(g):
    return None if g is None else g.contiguous(
        memory_format=torch.channels_last)


class _FusedBNFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var,
                momentum, eps, relu, residual, ws=None, pair=False):
        use_hip = x.is_cuda and ops_api.has_gpu_ops()
        assert not pair or (use_hip and relu and residual is not None)
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
        return _two_handles(ctx, y) if pair else y

    @staticmethod
    def backward(ctx, dy, dy_b=None):
        # sign: y itself, or on the HIP path with relu its packed y > 0 mask
        x, sign, save_mean, save_rstd, weight = ctx.saved_tensors
        relu, has_res = ctx.relu, ctx.has_res
        use_hip = x.is_cuda and ops_api.has_gpu_ops()
        if dy is None:  # pair: only the second handle was used, or neither
            dy, dy_b = dy_b, None
            if dy is None:
                return (None,) * 11
        if dy_b is not None:
            # pair, both handles used: the add happens in the reduce kernel,
            # and its masked sum dz is the residual's gradient
            dx, dweight, dbias, dres = ops_api.ext().bn_bwd_mask_join(
                x, _nhwc_grad(dy), _nhwc_grad(dy_b), sign, save_mean,
                save_rstd, weight, ctx.ws_bwd)
        elif use_hip:
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
        return (dx, dweight, dbias, None, None, None, None, None, dres, None,
                None)


class _FusedBNPoolFunction(torch.autograd.Function):
    """bn -> relu -> 3x3/stride 2/pad 1 max-pool on the HIP kernels. Saves x,
    the argmax words, the statistics and the weight: no full-resolution y."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, momentum,
                eps, ws):
        y, save_mean, save_rstd, argmax = ops_api.ext().bn_fwd_train_pool(
            x, weight, bias, running_mean, running_var, eps, momentum,
            ws[0] if ws is not None else None)
        ctx.ws_bwd = ws[1] if ws is not None else None
        ctx.save_for_backward(x, argmax, save_mean, save_rstd, weight)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, argmax, save_mean, save_rstd, weight = ctx.saved_tensors
        dx, dweight, dbias = ops_api.ext().bn_bwd_pool(
            x, dy.contiguous(memory_format=torch.channels_last), argmax,
            save_mean, save_rstd, weight, ctx.ws_bwd)
        return dx, dweight, dbias, None, None, None, None, None


class _FusedBNAddBNFunction(torch.autograd.Function):
    """relu(bn(z) + bn_d(zd)) with one apply kernel; backward is bn_bwd_mask
    on each branch, both with the dy and the packed mask of y. With `pair`
    and both handles used, the two-BN bn_bwd_mask_join adds the two gradients
    and runs both branches' backward on the masked sum in one reduce and one
    apply."""

    @staticmethod
    def forward(ctx, z, zd, weight, bias, running_mean, running_var, momentum,
                eps, ws, weight_d, bias_d, running_mean_d, running_var_d,
                momentum_d, eps_d, ws_d, pair=False):
        y, mask, sm, sr, sm_d, sr_d = ops_api.ext().bn_fwd_train_add_bn(
            z, zd, weight, bias, running_mean, running_var, eps, momentum,
            ws[0] if ws is not None else None,
            weight_d, bias_d, running_mean_d, running_var_d, eps_d,
            momentum_d, ws_d[0] if ws_d is not None else None)
        ctx.ws_bwd = ws[1] if ws is not None else None
        ctx.ws_bwd_d = ws_d[1] if ws_d is not None else None
        ctx.save_for_backward(z, zd, mask, sm, sr, sm_d, sr_d, weight,
                              weight_d)
        return _two_handles(ctx, y) if pair else y

    @staticmethod
    def backward(ctx, dy, dy_b=None):
        z, zd, mask, sm, sr, sm_d, sr_d, weight, weight_d = ctx.saved_tensors
        if dy is None:  # pair: only the second handle was used, or neither
            dy, dy_b = dy_b, None
            if dy is None:
                return (None,) * 17
        dy = _nhwc_grad(dy)
        if dy_b is not None:
            # the two-BN signature: one reduce forms the masked sum and the
            # sums of both branches, one apply reads it for dz and dzd
            dz, dw, db, _, dzd, dw_d, db_d = ops_api.ext().bn_bwd_mask_join(
                z, dy, _nhwc_grad(dy_b), mask, sm, sr, weight, ctx.ws_bwd,
                zd, sm_d, sr_d, weight_d, ctx.ws_bwd_d)
        else:
            bwd = ops_api.ext().bn_bwd_mask
            dz, dw, db = bwd(z, dy, mask, sm, sr, weight, True, False,
                             ctx.ws_bwd)
            dzd, dw_d, db_d = bwd(zd, dy, mask, sm_d, sr_d, weight_d, True,
                                  False, ctx.ws_bwd_d)
        return (dz, dzd, dw, db, None, None, None, None, None,
                dw_d, db_d, None, None, None, None, None, None)


def fused_bn_train(x, weight, bias, running_mean, running_var,
                   momentum=0.1, eps=1e-5, relu=False,
                   residual: Optional[torch.Tensor] = None, ws=None,
                   pair=False):
    """pair (HIP, relu and a residual only): returns two handles of y, see
    FusedBatchNorm2d.forward_add_pair."""
    return _FusedBNFunction.apply(x, weight, bias, running_mean, running_var,
                                  momentum, eps, relu, residual, ws, pair)


class FusedBatchNorm2d(torch.nn.Module):
    """Drop-in BatchNorm2d with optional fused ReLU and residual add.

    forward(x) applies bn [+relu]; forward_add(x, residual) applies
    bn(x) + residual -> relu (the Bottleneck tail); forward_pool(x) applies
    bn -> relu -> 3x3/2 max-pool (the ResNet stem); forward_add_bn(z, zd, bn_d)
    applies relu(bn(z) + bn_d(zd)) (the tail of a block with a downsample).

    forward_add_pair / forward_add_bn_pair are the two tails for a block
    output with two consumers: they return (y_main, y_res), two handles of
    the one y. Give each consumer its own handle and backward receives the
    two gradients apart and adds them inside its reduce kernel
    (bn_bwd_mask_join) instead of reading a sum that a stand-alone add wrote.
    Off the fused HIP path both handles are the same tensor and autograd adds.
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

    def _workspace(self, x):
        if not x.is_cuda:
            return None
        if self._ws is None or self._ws[0].device != x.device:
            # layouts match BN_GM_MAX=512 in csrc/ext.hip: reduce partials
            # plus scale/shift (fwd) and k1..k3 (bwd). Only values that are
            # dead when the call returns live here; save_mean/save_rstd come
            # back freshly allocated, so calling this module twice before
            # backward is safe.
            self._ws = (
                torch.empty(2 * 512 + 4, self.num_features, device=x.device),
                torch.empty(2 * 512 + 3, self.num_features, device=x.device))
        return self._ws

    def forward(self, x, residual: Optional[torch.Tensor] = None):
        x = self._check(x)
        if residual is not None:
            residual = self._check(residual)
        if self.training:
            self.num_batches_tracked += 1
            return fused_bn_train(x, self.weight, self.bias,
                                  self.running_mean, self.running_var,
                                  self.momentum, self.eps, self.relu, residual,
                                  ws=self._workspace(x))
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

    def _fused_kernels(self, x):
        return (self.training and x.is_cuda and ops_api.has_gpu_ops()
                and not SPLIT_PATH)

    def forward_add_pair(self, x, residual):
        """forward_add(x, residual) as (y_main, y_res)."""
        if not (self._fused_kernels(x) and self.relu):
            y = self.forward_add(x, residual)
            return y, y
        self.num_batches_tracked += 1
        return fused_bn_train(self._check(x), self.weight, self.bias,
                              self.running_mean, self.running_var,
                              self.momentum, self.eps, True,
                              self._check(residual), ws=self._workspace(x),
                              pair=True)

    def forward_pool(self, x):
        """max_pool2d(self(x), 3, 2, 1), the ResNet stem, without the
        full-resolution y: the apply kernel pools, backward gathers through
        the saved argmax words. The caller uses this in place of
        `pool(self(x))`, so forward hooks registered on this module (they
        hang on `__call__`) do not fire."""
        assert self.relu, "forward_pool is bn -> relu -> max-pool"
        if not self._fused_kernels(x):
            return torch.nn.functional.max_pool2d(self.forward(x), 3, 2, 1)
        x = self._check(x)
        self.num_batches_tracked += 1
        return _FusedBNPoolFunction.apply(
            x, self.weight, self.bias, self.running_mean, self.running_var,
            self.momentum, self.eps, self._workspace(x))

    def forward_add_bn_pair(self, z, zd, other_bn):
        """forward_add_bn(z, zd, other_bn) as (y_main, y_res)."""
        return self.forward_add_bn(z, zd, other_bn, pair=True)

    def forward_add_bn(self, z, zd, other_bn, pair=False):
        """relu(self_bn(z) + other_bn(zd)): the tail of a block whose identity
        branch ends in a ReLU-less BN (`other_bn`), with one apply kernel and
        no stored identity tensor. `other_bn` is handed over, not called:
        forward hooks on it, on this module and on a Sequential that holds
        `other_bn` do not fire on this path."""
        if not (self._fused_kernels(z) and self.relu
                and isinstance(other_bn, FusedBatchNorm2d)
                and other_bn.training and not other_bn.relu):
            y = self.forward_add(z, other_bn(zd))
            return (y, y) if pair else y
        z, zd = self._check(z), other_bn._check(zd)
        self.num_batches_tracked += 1
        other_bn.num_batches_tracked += 1
        return _FusedBNAddBNFunction.apply(
            z, zd, self.weight, self.bias, self.running_mean,
            self.running_var, self.momentum, self.eps, self._workspace(z),
            other_bn.weight, other_bn.bias, other_bn.running_mean,
            other_bn.running_var, other_bn.momentum, other_bn.eps,
            other_bn._workspace(zd), pair)

    def extra_repr(self):
        return f"{self.num_features}, relu={self.relu}"
