"""The block-input gradient add folded into the tail BN's backward.

A residual block's output has two consumers, so its gradient arrives as two
addends. bn_bwd_mask_join(x, dy_a, dy_b, mask, ...) forms
dz = mask ? T(dy_a + dy_b) : 0 inside its reduce kernel, stores it, and runs
the plain apply kernel on it. The split path it replaces is run in the same
test: s = dy_a + dy_b by torch, then bn_bwd_mask(x, s, mask, need_dres=True).
The add is one fp32 add rounded to T on both paths, the sums are taken from
the same values in the same order and dz is that path's dres, so every check
is torch.equal, not a bound. The addends are randn, not integers: more than
half of their bf16 sums have to round, which the tests assert first.
"""
import functools

import pytest
import torch

from tests.test_bn_geometry_gpu import (  # noqa: F401 - ext is a fixture
    EPS, _inputs, _make_ws, _nhwc, ext)
from tests.test_bn_mask_gpu import DTYPES, SHAPES

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(C, M, dtype):
    """Forward with a residual (mask and statistics), the two addends, and
    the split path's backward on their torch sum; computed once per shape and
    shared read-only."""
    from autodist_amd.ops import api
    e = api.ext()
    x, res, _, w, b, rm, rv = _inputs(C, M, dtype, True, seed=C + M)
    g = torch.Generator(device="cuda").manual_seed(C + M + 2)
    a = torch.randn(M, C, generator=g, device="cuda").to(dtype)
    bb = torch.randn(M, C, generator=g, device="cuda").to(dtype)
    zd = torch.randn(M, C, generator=g, device="cuda").to(dtype)
    wd = torch.rand(C, generator=g, device="cuda") + 0.5
    bd = torch.randn(C, generator=g, device="cuda")
    y4, sm, sr, mask = e.bn_fwd_train_mask(_nhwc(x), w, b, rm, rv, _nhwc(res),
                                           EPS, 0.1, True, None)
    # statistics of a second, ReLU-less BN on zd (the downsample branch)
    _, smd, srd = e.bn_fwd_train(_nhwc(zd), wd, bd, rm.clone(), rv.clone(),
                                 None, EPS, 0.1, False, None)
    s = a + bb
    ref = e.bn_bwd_mask(_nhwc(x), _nhwc(s), mask, sm, sr, w, True, True,
                        _make_ws(C, "persistent")[1])
    ref_d = e.bn_bwd_mask(_nhwc(zd), _nhwc(s), mask, smd, srd, wd, True,
                          False, _make_ws(C, "persistent")[1])
    return dict(x=x, a=a, b=bb, s=s, zd=zd, w=w, wd=wd, sm=sm, sr=sr, smd=smd,
                srd=srd, mask=mask, ref=ref, ref_d=ref_d)


def _not_vacuous(f, dtype):
    """The sums round, ties occur or not (printed), both mask bits occur."""
    exact = f["a"].float() + f["b"].float()
    if dtype == torch.bfloat16:
        inexact = (f["s"].float() != exact).float().mean().item()
        # a tie: the fp32 sum lies halfway between two bf16 values, i.e. its
        # low 16 bits are exactly 0x8000
        low = exact.view(torch.int32) & 0xFFFF
        ties = (low == 0x8000).float().mean().item()
        print(f"share of sums that round: {inexact:.3f}, exact ties: "
              f"{ties:.5f}")
        assert inexact > 0.4, inexact
    ones = int(f["mask"].to(torch.int32).bitwise_and(0xFF).ne(0).sum())
    zeros = int(f["mask"].ne(0xFF).sum())
    assert ones > 0 and zeros > 0, "the mask must hold zeros and ones"


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,M", SHAPES, ids=[f"C{c}-M{m}" for c, m in SHAPES])
def test_join_equals_add_then_mask_bwd(ext, C, M, dtype):
    f = _case(C, M, dtype)
    _not_vacuous(f, dtype)
    out = ext.bn_bwd_mask_join(_nhwc(f["x"]), _nhwc(f["a"]), _nhwc(f["b"]),
                               f["mask"], f["sm"], f["sr"], f["w"],
                               _make_ws(C, "persistent")[1])
    assert len(out) == 4
    for name, got, ref in zip(("dx", "dweight", "dbias", "dz vs dres"), out,
                              f["ref"]):
        assert got.shape == ref.shape and got.dtype == ref.dtype, name
        assert torch.equal(got, ref), name
    # no workspace given: the same
    out2 = ext.bn_bwd_mask_join(_nhwc(f["x"]), _nhwc(f["a"]), _nhwc(f["b"]),
                                f["mask"], f["sm"], f["sr"], f["w"], None)
    for got, ref in zip(out2, f["ref"]):
        assert torch.equal(got, ref)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,M", SHAPES, ids=[f"C{c}-M{m}" for c, m in SHAPES])
def test_join_feeds_the_downsample_branch(ext, C, M, dtype):
    """add_bn tail: join on z, then the mask-less bn_bwd on zd with dz,
    against bn_bwd_mask on z and on zd, both with the torch sum."""
    f = _case(C, M, dtype)
    _not_vacuous(f, dtype)
    dz, dw, db, dym = ext.bn_bwd_mask_join(
        _nhwc(f["x"]), _nhwc(f["a"]), _nhwc(f["b"]), f["mask"], f["sm"],
        f["sr"], f["w"], _make_ws(C, "persistent")[1])
    dzd, dwd, dbd = ext.bn_bwd(_nhwc(f["zd"]), dym, dym, f["smd"], f["srd"],
                               f["wd"], False, False,
                               _make_ws(C, "persistent")[1])
    assert torch.equal(dz, f["ref"][0]), "dz"
    assert torch.equal(dw, f["ref"][1]) and torch.equal(db, f["ref"][2])
    assert torch.equal(dzd, f["ref_d"][0]), "dzd"
    assert torch.equal(dwd, f["ref_d"][1]), "dweight_d"
    assert torch.equal(dbd, f["ref_d"][2]), "dbias_d"


def test_join_rejects_mismatched_addends(ext):
    f = _case(24, 1000, torch.bfloat16)
    x4, a4 = _nhwc(f["x"]), _nhwc(f["a"])
    args = (f["mask"], f["sm"], f["sr"], f["w"], None)
    with pytest.raises(RuntimeError):
        ext.bn_bwd_mask_join(x4, a4, _nhwc(f["b"].float()), *args)
    with pytest.raises(RuntimeError):
        ext.bn_bwd_mask_join(x4, a4, _nhwc(f["b"][:-1]), *args)
    with pytest.raises(RuntimeError):
        ext.bn_bwd_mask_join(x4, a4, a4.contiguous(), *args)  # NCHW strides
    with pytest.raises(RuntimeError):
        ext.bn_bwd_mask_join(x4, a4.cpu(), a4, *args)


# ------------------------------------------------------------- model level
class _Counter:
    """Counts calls of ext.bn_bwd_mask_join while it is in place."""

    def __init__(self, e):
        self.e, self.orig, self.calls = e, e.bn_bwd_mask_join, 0

    def __enter__(self):
        def counted(*args):
            self.calls += 1
            return self.orig(*args)
        self.e.bn_bwd_mask_join = counted
        return self

    def __exit__(self, *exc):
        self.e.bn_bwd_mask_join = self.orig


def _make_chain(kind):
    from autodist_amd.models import resnet
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d
    cls = resnet.Bottleneck if kind == "bottleneck" else resnet.BasicBlock
    out_ch = 16 * cls.expansion
    ds = torch.nn.Sequential(
        torch.nn.Conv2d(32, out_ch, 1, stride=2, bias=False),
        FusedBatchNorm2d(out_ch, relu=False))
    chain = torch.nn.ModuleList([
        cls(32, 16, stride=2, downsample=ds, fused=True),
        cls(out_ch, 16, fused=True), cls(out_ch, 16, fused=True)])
    chain = chain.cuda().to(memory_format=torch.channels_last).train()
    with torch.no_grad():
        for m in chain.modules():
            if isinstance(m, FusedBatchNorm2d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_()
    return chain, out_ch


def _chain_grads(ext, chain, x, dy, split):
    from autodist_amd.ops import fused_bn
    chain.zero_grad(set_to_none=True)
    xa = x.detach().clone().requires_grad_(True)
    fused_bn.SPLIT_PATH = split
    try:
        with _Counter(ext) as n:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                xs = (xa, xa)
                for block in chain:
                    xs = block.forward_pair(xs)
                assert (xs[0] is xs[1]) == split
                assert xs[0].data_ptr() == xs[1].data_ptr()
            xs[0].backward(dy)
    finally:
        fused_bn.SPLIT_PATH = False
    bufs = {k: v.clone() for k, v in chain.named_buffers()}
    return (xs[0].detach(), xa.grad,
            [p.grad.clone() for p in chain.parameters()], bufs, n.calls)


@pytest.mark.parametrize("nhwc_grad", [True, False], ids=["nhwc", "nchw"])
@pytest.mark.parametrize("kind", ["bottleneck", "basic"])
def test_block_chain_equals_split_path(ext, kind, nhwc_grad):
    """Downsample block, then two identity blocks. The outputs of blocks 0
    and 1 have two consumers each: two joins. Block 2's output has one (its
    y_res is dropped): the bn_bwd_mask path. nchw: the gradient fed in is not
    channels_last."""
    det =torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        torch.manual_seed(2)
        chain, out_ch = _make_chain(kind)
        state = {k: v.clone() for k, v in chain.state_dict().items()}
        x = torch.randn(4, 32, 10, 10, device="cuda").contiguous(
            memory_format=torch.channels_last)
        dy = torch.randn(4, out_ch, 5, 5, device="cuda").to(torch.bfloat16)
        if nhwc_grad:
            dy = dy.contiguous(memory_format=torch.channels_last)
        else:
            assert not dy.is_contiguous(memory_format=torch.channels_last)
        new = _chain_grads(ext, chain, x, dy, split=False)
        chain.load_state_dict(state)
        old = _chain_grads(ext, chain, x, dy, split=True)
    finally:
        torch.backends.cudnn.deterministic = det
    assert new[4] == 2 and old[4] == 0, (new[4], old[4])
    assert torch.equal(new[0], old[0]), "output"
    assert torch.equal(new[1], old[1]), "dx"
    for (name, _), a, c in zip(chain.named_parameters(), new[2], old[2]):
        assert torch.equal(a, c), name
    for k in new[3]:
        assert torch.equal(new[3][k], old[3][k]), k


@pytest.mark.parametrize("use", ["main", "res"])
def test_one_handle_unused_equals_forward_add(ext, use):
    """A single tail whose other handle is dropped: backward gets one
    gradient and None, takes the bn_bwd_mask path and gives forward_add's
    gradients."""
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d
    C, M = 48, 1000
    x, res, _, w, b, _, _ = _inputs(C, M, torch.bfloat16, True, seed=21)
    g = torch.Generator(device="cuda").manual_seed(22)
    dy = _nhwc(torch.randn(M, C, generator=g, device="cuda").bfloat16())
    bn = FusedBatchNorm2d(C, relu=True).cuda().train()
    with torch.no_grad():
        bn.weight.copy_(w)
        bn.bias.copy_(b)
    state = {k: v.clone() for k, v in bn.state_dict().items()}
    outs = []
    for pair in (False, True):
        bn.load_state_dict(state)
        bn.zero_grad(set_to_none=True)
        xa = _nhwc(x).detach().requires_grad_(True)
        ra = _nhwc(res).detach().requires_grad_(True)
        with _Counter(ext) as n:
            if pair:
                ys = bn.forward_add_pair(xa, ra)
                assert ys[0] is not ys[1]
                y = ys[0] if use == "main" else ys[1]
                del ys
            else:
                y = bn.forward_add(xa, ra)
            y.backward(dy)
        assert n.calls == 0
        outs.append((y.detach(), xa.grad, ra.grad, bn.weight.grad.clone(),
                     bn.bias.grad.clone(), bn.running_mean.clone(),
                     bn.running_var.clone()))
    for name, a, c in zip(("y", "dx", "dres", "dweight", "dbias", "rm", "rv"),
                          *outs):
        assert torch.equal(a, c), name
