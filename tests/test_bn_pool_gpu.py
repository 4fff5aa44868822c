"""Fused bn -> relu -> 3x3/stride 2/pad 1 max-pool (the ResNet stem).

bn_fwd_train_pool returns the pooled y and one argmax word per pooled pixel
and 8 channels; bn_bwd_pool gathers dz through those words. The reference is
the split path run in the same test, whose kernels have tests of their own:
    bn_fwd_train_mask -> F.max_pool2d -> its autograd backward -> bn_bwd_mask
The fused path forms the same rounded values, keeps the first maximum like
torch does and adds the at most four pooled gradients of an input pixel in
fp32 before it rounds once, so every check here is an equality:
  * pooled y, save_mean, save_rstd and both running statistics;
  * every argmax nibble against the reference's full-resolution y;
  * dx, dweight and dbias with integer dy in [-4, 4] (sums of up to four of
    them are exact in bf16 and fp32), and dbias against the integer column
    sum taken in float64.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.test_bn_geometry_gpu import (  # noqa: F401 - ext is a fixture
    BN_VEC, EPS, _make_ws, ext)

pytestmark = pytest.mark.gpu

# (N, C, H, W)
SHAPES = [
    (1, 8, 1, 1),        # one pixel, a window with one valid position
    (2, 8, 5, 7),        # odd sizes, every border case
    (3, 24, 8, 8),       # even sizes, tx_count 3
    (2, 64, 12, 10),     # the stem's channel count
    (1, 80, 33, 17),     # leftover threads
    (2, 2056, 4, 4),     # grid_c = 2
    # M = 150 528 rows > 4096 blocks x 32 rows: the grid-stride loops run
    (3, 64, 224, 224),
]
DTYPES = [torch.bfloat16, torch.float32]
NONE = 15


def _cl(t):
    return t.contiguous(memory_format=torch.channels_last)


def _inputs(N, C, H, W, dtype, seed, ties=False):
    g = torch.Generator(device="cuda").manual_seed(seed)
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    if ties:
        # integers in [-3, 3], the larger of two uniform draws: a single
        # uniform draw gives nine-position windows a tied positive maximum
        # in 52 % of the cases only (and border windows fewer); with 26 %
        # of the values at 3 it is three in four
        ri = lambda: torch.randint(-3, 4, (N, C, H, W), generator=g,  # noqa
                                   device="cuda")
        x = torch.maximum(ri(), ri()).to(dtype)
        w = torch.ones(C, device="cuda")
        b = torch.zeros(C, device="cuda")
    else:
        x = torch.randn(N, C, H, W, generator=g, device="cuda").to(dtype)
        w = torch.rand(C, generator=g, device="cuda") + 0.5
        b = torch.randn(C, generator=g, device="cuda") * 0.5
    dy = torch.randint(-4, 5, (N, C, Ho, Wo), generator=g,
                       device="cuda").to(dtype)
    rm = torch.randn(C, generator=g, device="cuda")
    rv = torch.rand(C, generator=g, device="cuda") + 0.5
    return _cl(x), _cl(dy), w, b, rm, rv


@functools.lru_cache(maxsize=None)
def _both(N, C, H, W, dtype, ties=False):
    """Split path and fused path on the same seeded inputs, on NaN-filled
    workspaces of their own; computed once per case and left unchanged."""
    from autodist_amd.ops import api
    e = api.ext()
    x, dy, w, b, rm, rv = _inputs(N, C, H, W, dtype, N + C + H + W, ties)
    r = dict(x=x, dy=dy, w=w)
    # reference
    rm_r, rv_r = rm.clone(), rv.clone()
    ws_f, ws_b = _make_ws(C, "persistent")
    y4, sm, sr, mask = e.bn_fwd_train_mask(x, w, b, rm_r, rv_r, None, EPS,
                                           0.1, True, ws_f)
    ya = y4.detach().requires_grad_(True)
    yp = F.max_pool2d(ya, 3, 2, 1)
    yp.backward(dy)
    dy_full = _cl(ya.grad)
    dx, dw, db = e.bn_bwd_mask(x, dy_full, mask, sm, sr, w, True, False, ws_b)
    r.update(y_full=y4, yp_r=yp.detach(), sm_r=sm, sr_r=sr, rm_r=rm_r,
             rv_r=rv_r, dy_full=dy_full, dx_r=dx, dw_r=dw, db_r=db)
    # fused
    rm_f, rv_f = rm.clone(), rv.clone()
    ws_f, ws_b = _make_ws(C, "persistent")
    yp_f, sm_f, sr_f, amax = e.bn_fwd_train_pool(x, w, b, rm_f, rv_f, EPS,
                                                 0.1, ws_f)
    dx_f, dw_f, db_f = e.bn_bwd_pool(x, dy, amax, sm_f, sr_f, w, ws_b)
    r.update(yp_f=yp_f, sm_f=sm_f, sr_f=sr_f, rm_f=rm_f, rv_f=rv_f,
             amax=amax, dx_f=dx_f, dw_f=dw_f, db_f=db_f)
    return r


def _nibbles(amax, N, C, Ho, Wo):
    """[N*Ho*Wo, C/8] int32 -> [N, C, Ho, Wo] window positions."""
    assert amax.dtype == torch.int32 and amax.is_contiguous()
    assert amax.shape == (N * Ho * Wo, C // BN_VEC)
    k = torch.arange(BN_VEC, device=amax.device, dtype=torch.int32)
    nib = (amax.unsqueeze(-1) >> (4 * k)) & 15
    return nib.reshape(N, Ho, Wo, C).permute(0, 3, 1, 2)


def _windows(y, Ho, Wo):
    """[9, N, C, Ho, Wo]: the full-resolution y at window position kh*3+kw of
    every pooled pixel, -inf outside the image."""
    yp = F.pad(y.float(), (1, 1, 1, 1), value=float("-inf"))
    return torch.stack([yp[:, :, kh:kh + 2 * Ho - 1:2, kw:kw + 2 * Wo - 1:2]
                        for kh in range(3) for kw in range(3)])


def _check(r, N, C, H, W):
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert r["yp_f"].shape == (N, C, Ho, Wo)
    assert r["yp_f"].is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(r["yp_f"], r["yp_r"]), "pooled y"
    assert torch.equal(r["sm_f"], r["sm_r"]), "save_mean"
    assert torch.equal(r["sr_f"], r["sr_r"]), "save_rstd"
    assert torch.equal(r["rm_f"], r["rm_r"]), "running_mean"
    assert torch.equal(r["rv_f"], r["rv_r"]), "running_var"
    # argmax words against the reference's full-resolution y
    win = _windows(r["y_full"], Ho, Wo)
    pooled = r["yp_r"].float()
    nib = _nibbles(r["amax"], N, C, Ho, Wo).long()
    live = pooled > 0
    assert torch.equal(nib == NONE, ~live), "nibble 15 <=> pooled value <= 0"
    assert int(nib[live].max() if live.any() else 0) <= 8
    named = win.gather(0, nib.clamp(max=8).unsqueeze(0))[0]
    assert torch.equal(named[live], pooled[live]), \
        "a nibble names a position outside the image or not at the maximum"
    pos = torch.arange(9, device="cuda").view(9, 1, 1, 1, 1)
    first = torch.where(win == pooled, pos, 9).min(0).values
    assert torch.equal(nib[live], first[live]), "not the first maximum"
    # backward
    assert torch.equal(r["dx_f"], r["dx_r"]), "dx"
    assert torch.equal(r["dw_f"], r["dw_r"]), "dweight"
    assert torch.equal(r["db_f"], r["db_r"]), "dbias"
    dz = r["dy_full"].double() * (r["y_full"] > 0)
    col = dz.sum((0, 2, 3))
    assert dz.abs().sum((0, 2, 3)).max().item() < 2 ** 24
    assert torch.equal(r["db_f"], col.float()), "dbias != integer column sum"
    return win, pooled


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("shape", SHAPES,
                         ids=["x".join(map(str, s)) for s in SHAPES])
def test_pool_equals_split_path(ext, shape, dtype):
    _check(_both(*shape, dtype), *shape)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_pool_ties_take_the_first_maximum(ext, dtype):
    shape = (2, 64, 12, 10)
    win, pooled = _check(_both(*shape, dtype, ties=True), *shape)
    tied = ((win == pooled).sum(0) >= 2) & (pooled > 0)
    frac = tied.float().mean().item()
    print(f"windows with a tied positive maximum: {frac:.3f}")
    assert frac > 0.5


# ------------------------------------------------------------------ wrapper
def _module(C=16):
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d
    bn = FusedBatchNorm2d(C, relu=True).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    return bn


def test_forward_pool_saves_no_full_resolution_y(ext):
    bn = _module()
    g = torch.Generator(device="cuda").manual_seed(3)
    x = _cl(torch.randn(2, 16, 9, 12, generator=g, device="cuda")
            .to(torch.bfloat16)).requires_grad_(True)
    y = bn.forward_pool(x)
    assert y.shape == (2, 16, 5, 6)
    saved = y.grad_fn.saved_tensors
    assert saved[0].data_ptr() == x.data_ptr()
    assert saved[1].dtype == torch.int32 and saved[1].shape == (2 * 5 * 6, 2)
    for t in saved[1:]:
        assert t.numel() * t.element_size() < x.numel() * x.element_size() // 4
    assert int(bn.num_batches_tracked) == 1
    # and it is the module's own forward followed by the pool
    bn2 = _module()
    bn2.load_state_dict({k: v for k, v in bn.state_dict().items()})
    with torch.no_grad():
        bn2.running_mean.zero_()
        bn2.running_var.fill_(1.0)
        bn2.num_batches_tracked.zero_()
    x2 = x.detach().clone().requires_grad_(True)
    y2 = F.max_pool2d(bn2(x2), 3, 2, 1)
    dy = torch.randint(-4, 5, y.shape, generator=g, device="cuda").to(y.dtype)
    y.backward(_cl(dy))
    y2.backward(_cl(dy))
    assert torch.equal(y, y2) and torch.equal(x.grad, x2.grad)
    assert torch.equal(bn.weight.grad, bn2.weight.grad)
    assert torch.equal(bn.bias.grad, bn2.bias.grad)
    assert torch.equal(bn.running_mean, bn2.running_mean)
    assert torch.equal(bn.running_var, bn2.running_var)


def test_module_twice_each_backward_has_its_own_argmax(ext):
    bn = _module()
    g = torch.Generator(device="cuda").manual_seed(5)
    mk = lambda s, o: _cl((torch.randn(2, 16, 9, 12, generator=g,  # noqa
                                       device="cuda") * s + o)
                          .to(torch.bfloat16))
    xs = [mk(1.0, 0.0).requires_grad_(True), mk(2.0, 1.0).requires_grad_(True)]
    gs = [_cl(torch.randint(-4, 5, (2, 16, 5, 6), generator=g, device="cuda")
              .to(torch.bfloat16)) for _ in range(2)]
    w, b = bn.weight.detach().clone(), bn.bias.detach().clone()
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    direct = []
    for x, dy in zip(xs, gs):
        yp, sm, sr, amax = ext.bn_fwd_train_pool(x.detach(), w, b, rm, rv,
                                                 bn.eps, bn.momentum, None)
        direct.append((yp, ext.bn_bwd_pool(x.detach(), dy, amax, sm, sr, w,
                                           None)))
    ys = [bn.forward_pool(xs[0]), bn.forward_pool(xs[1])]
    words = [y.grad_fn.saved_tensors[1] for y in ys]
    assert words[0].data_ptr() != words[1].data_ptr()
    assert not torch.equal(words[0], words[1])
    for a in words:
        for t in bn._ws:
            lo = t.data_ptr()
            assert not lo <= a.data_ptr() < lo + t.numel() * t.element_size()
    torch.autograd.backward(ys, gs)
    for i in range(2):
        assert torch.equal(ys[i], direct[i][0])
        assert torch.equal(xs[i].grad, direct[i][1][0])
    assert torch.equal(bn.weight.grad, direct[0][1][1] + direct[1][1][1])
    assert torch.equal(bn.bias.grad, direct[0][1][2] + direct[1][1][2])
    assert torch.equal(bn.running_mean, rm)
    assert torch.equal(bn.running_var, rv)


def test_resnet50_stem_equals_the_old_path(ext):
    from autodist_amd.models.resnet import resnet50
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(0)
        model = resnet50(num_classes=10, fused=True).cuda().to(
            memory_format=torch.channels_last).train()
        state = {k: v.clone() for k, v in model.state_dict().items()}
        x = _cl(torch.randn(2, 3, 64, 64, device="cuda"))
        t = torch.tensor([1, 7], device="cuda")

        def run():
            model.load_state_dict(state)
            model.zero_grad(set_to_none=True)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = F.cross_entropy(model(x), t)
            loss.backward()
            return loss.detach().clone(), [p.grad.clone()
                                           for p in model.parameters()]

        new = run()
        assert model.bn1._ws is not None
        # the stem through bn -> F.max_pool2d, everything else as it was
        model.bn1.forward_pool = lambda v: model.maxpool(model.bn1(v))
        old = run()
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(new[0], old[0]), (new[0], old[0])
    for (name, _), a, c in zip(model.named_parameters(), new[1], old[1]):
        assert torch.equal(a, c), name
