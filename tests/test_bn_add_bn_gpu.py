"""Block tail with a batch-normed identity: y = relu(bn3(z) + bn_ds(zd)).

bn_fwd_train_add_bn runs both BNs' statistics and one apply kernel; backward
is bn_bwd_mask on each branch with the dy and the packed mask of y. The
reference is the split path run in the same test:
    bn_fwd_train(zd) -> identity; bn_fwd_train_mask(z, residual=identity);
    bn_bwd_mask(..., need_dres=True) -> dz, dres; bn_bwd(zd, dres)
The joint apply kernel rounds the inner BN to T as the stored identity was,
and dres is dz, so every output must be torch.equal (integer dy keeps the
column sums exact, as in tests/test_bn_geometry_gpu.py).
"""
import functools

import pytest
import torch

from tests.test_bn_geometry_gpu import (  # noqa: F401 - ext is a fixture
    EPS, _inputs, _make_ws, _nhwc, ext)
from tests.test_bn_mask_gpu import DTYPES, SHAPES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _both(C, M, dtype):
    from autodist_amd.ops import api
    e = api.ext()
    z, zd, dy, w, b, rm, rv = _inputs(C, M, dtype, True, seed=C + M)
    g = torch.Generator(device="cuda").manual_seed(C + M + 1)
    wd = torch.rand(C, generator=g, device="cuda") + 0.5
    bd = torch.randn(C, generator=g, device="cuda")
    rmd = torch.randn(C, generator=g, device="cuda")
    rvd = torch.rand(C, generator=g, device="cuda") + 0.5
    z4, zd4, dy4 = _nhwc(z), _nhwc(zd), _nhwc(dy)
    # split path
    s = dict(rm=rm.clone(), rv=rv.clone(), rmd=rmd.clone(), rvd=rvd.clone())
    ws3, wsd = _make_ws(C, "persistent"), _make_ws(C, "persistent")
    ident, s["smd"], s["srd"] = e.bn_fwd_train(
        zd4, wd, bd, s["rmd"], s["rvd"], None, EPS, 0.2, False, wsd[0])
    s["y"], s["sm"], s["sr"], s["mask"] = e.bn_fwd_train_mask(
        z4, w, b, s["rm"], s["rv"], ident, EPS, 0.1, True, ws3[0])
    s["dz"], s["dw"], s["db"], dres = e.bn_bwd_mask(
        z4, dy4, s["mask"], s["sm"], s["sr"], w, True, True, ws3[1])
    s["dzd"], s["dwd"], s["dbd"] = e.bn_bwd(
        zd4, dres, ident, s["smd"], s["srd"], wd, False, False, wsd[1])
    # joint path
    j = dict(rm=rm.clone(), rv=rv.clone(), rmd=rmd.clone(), rvd=rvd.clone())
    ws3, wsd = _make_ws(C, "persistent"), _make_ws(C, "persistent")
    j["y"], j["mask"], j["sm"], j["sr"], j["smd"], j["srd"] = \
        e.bn_fwd_train_add_bn(z4, zd4, w, b, j["rm"], j["rv"], EPS, 0.1,
                              ws3[0], wd, bd, j["rmd"], j["rvd"], EPS, 0.2,
                              wsd[0])
    j["dz"], j["dw"], j["db"] = e.bn_bwd_mask(
        z4, dy4, j["mask"], j["sm"], j["sr"], w, True, False, ws3[1])
    j["dzd"], j["dwd"], j["dbd"] = e.bn_bwd_mask(
        zd4, dy4, j["mask"], j["smd"], j["srd"], wd, True, False, wsd[1])
    return s, j


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,M", SHAPES, ids=[f"C{c}-M{m}" for c, m in SHAPES])
def test_add_bn_forward_equals_split_path(ext, C, M, dtype):
    s, j = _both(C, M, dtype)
    for k in ("y", "mask", "sm", "sr", "smd", "srd", "rm", "rv", "rmd",
              "rvd"):
        assert torch.equal(j[k], s[k]), k
    assert 0 < int((s["y"] > 0).sum()) < s["y"].numel()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,M", SHAPES, ids=[f"C{c}-M{m}" for c, m in SHAPES])
def test_add_bn_backward_equals_split_path(ext, C, M, dtype):
    s, j = _both(C, M, dtype)
    for k in ("dw", "db", "dwd", "dbd", "dz", "dzd"):
        assert torch.equal(j[k], s[k]), k


# ------------------------------------------------------------- model level
def _block_grads(block, x, dy, split):
    from autodist_amd.ops import fused_bn
    block.zero_grad(set_to_none=True)
    xa = x.detach().clone().requires_grad_(True)
    fused_bn.SPLIT_PATH = split
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = block(xa)
        y.backward(dy)
    finally:
        fused_bn.SPLIT_PATH = False
    bufs = {k: v.clone() for k, v in block.named_buffers()}
    return y.detach(), xa.grad, [p.grad.clone()
                                 for p in block.parameters()], bufs


@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_block_with_downsample_equals_split_path(ext, kind):
    from autodist_amd.models import resnet
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(1)
        cls = resnet.Bottleneck if kind == "bottleneck" else resnet.BasicBlock
        out_ch = 16 * cls.expansion
        ds = torch.nn.Sequential(
            torch.nn.Conv2d(32, out_ch, 1, stride=2, bias=False),
            FusedBatchNorm2d(out_ch, relu=False))
        block = cls(32, 16, stride=2, downsample=ds, fused=True).cuda().to(
            memory_format=torch.channels_last).train()
        with torch.no_grad():
            for m in block.modules():
                if isinstance(m, FusedBatchNorm2d):
                    m.weight.uniform_(0.5, 1.5)
                    m.bias.normal_()
        state = {k: v.clone() for k, v in block.state_dict().items()}
        x = torch.randn(4, 32, 10, 10, device="cuda").contiguous(
            memory_format=torch.channels_last)
        dy = torch.randint(-4, 5, (4, out_ch, 5, 5), device="cuda").to(
            torch.bfloat16).contiguous(memory_format=torch.channels_last)
        new = _block_grads(block, x, dy, split=False)
        block.load_state_dict(state)
        old = _block_grads(block, x, dy, split=True)
    finally:
        torch.backends.cudnn.deterministic = det
    assert torch.equal(new[0], old[0]), "output"
    assert torch.equal(new[1], old[1]), "dx"
    for (name, _), a, c in zip(block.named_parameters(), new[2], old[2]):
        assert torch.equal(a, c), name
    for k in new[3]:
        assert torch.equal(new[3][k], old[3][k]), k
    assert int(ds[1].num_batches_tracked) == 1
