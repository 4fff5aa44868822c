"""Fused BN: the bit-packed ReLU mask and the unrolled reduce / finalize loops.

bn_fwd_train_mask returns, beside what bn_fwd_train returns, a uint8 mask
[M, C/8]: bit k of byte (m, c0/8) is set iff the stored y[m, c0+k] > 0.
bn_bwd_mask takes that mask where bn_bwd takes y. Nothing else differs, so
every check here is an equality, not a bound:
  * the unpacked mask is torch.equal to y > 0, and the other outputs of the
    two forward entry points are torch.equal;
  * every output of bn_bwd_mask is torch.equal to bn_bwd's given the same y
    (the y path is what tests/test_bn_geometry_gpu.py bounds against
    float64);
  * with integer dy (and integer x) the column sums are exact in fp32, so a
    row that an unrolled loop or its tail drops or adds twice fails outright.
The reduce kernels issue the loads of BN_RED_U rows per trip and the finalize
kernels those of BN_FIN_U partial rows; both constants are read from the
extension and the tail shapes below are derived from them.
"""
import functools

import pytest
import torch

from tests.test_bn_geometry_gpu import (  # noqa: F401 - ext is a fixture
    BN_VEC, EPS, FIN_LANES, GM_MAX, _flat, _geom, _inputs, _make_ws,
    _nhwc, _two_inputs, ext)

pytestmark = pytest.mark.gpu

# (C, M): one thread column and fewer rows than a block; leftover threads
# (tx_count 3 and 10); grid-stride loop with a ragged tail; grid_c = 2
SHAPES = [(8, 3), (24, 1000), (80, 1000), (64, 6149), (2056, 70)]
DTYPES = [torch.bfloat16, torch.float32]


def _unpack(mask, C):
    """[M, C/8] uint8 -> [M, C] bool, bit k of a byte = channel c0 + k."""
    assert mask.dtype == torch.uint8 and mask.dim() == 2
    assert mask.size(1) * BN_VEC == C and mask.is_contiguous()
    k = torch.arange(BN_VEC, device=mask.device, dtype=torch.int32)
    bits = (mask.to(torch.int32).unsqueeze(-1) >> k) & 1
    return bits.bool().reshape(mask.size(0), C)


@functools.lru_cache(maxsize=None)
def _forward(C, M, dtype, residual):
    """Both forward entry points on the same seeded inputs, computed once
    per shape and shared (read-only) by the tests below."""
    from autodist_amd.ops import api
    e = api.ext()
    x, res, dy, w, b, rm, rv = _inputs(C, M, dtype, residual, seed=C + M)
    r4 = _nhwc(res) if residual else None
    rm_y, rv_y, rm_m, rv_m = rm.clone(), rv.clone(), rm.clone(), rv.clone()
    y4, sm, sr = e.bn_fwd_train(_nhwc(x), w, b, rm_y, rv_y, r4, EPS, 0.1,
                                True, None)
    out = e.bn_fwd_train_mask(_nhwc(x), w, b, rm_m, rv_m, r4, EPS, 0.1, True,
                              None)
    assert len(out) == 4
    return dict(x=x, dy=dy, w=w, y4=y4, sm=sm, sr=sr, rm=rm_y, rv=rv_y,
                y4_m=out[0], sm_m=out[1], sr_m=out[2], mask=out[3], rm_m=rm_m,
                rv_m=rv_m)


@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,M", SHAPES, ids=[f"C{c}-M{m}" for c, m in SHAPES])
def test_mask_is_y_gt_0(ext, C, M, dtype, residual):
    f = _forward(C, M, dtype, residual)
    assert f["mask"].shape == (M, C // BN_VEC)
    y = _flat(f["y4_m"])
    assert torch.equal(_unpack(f["mask"], C), y > 0)
    assert 0 < int((y > 0).sum()) < y.numel()  # both bit values occur
    assert torch.equal(f["y4_m"], f["y4"])
    assert torch.equal(f["sm_m"], f["sm"]) and torch.equal(f["sr_m"], f["sr"])
    assert torch.equal(f["rm_m"], f["rm"]) and torch.equal(f["rv_m"], f["rv"])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_mask_zeros_and_negatives(ext, dtype):
    """Channels 0..7 have weight = bias = 0, so bn(x) is 0 there and y is
    relu(residual) with the residual cycling through 0.0, -0.0, negatives and
    positives: the bit must be y > 0, not y >= 0 and not the sign bit."""
    C, M = 24, 1000
    x, res, dy, w, b, rm, rv = _inputs(C, M, dtype, True, seed=17)
    w[:BN_VEC] = 0.0
    b[:BN_VEC] = 0.0
    pat = torch.tensor([0.0, -0.0, -1.5, 2.0, -0.0, 0.0, 0.25, -3.0],
                       device="cuda")
    # res[m, k] = pat[(m + k) % 8]: every value meets every bit position
    idx = (torch.arange(M, device="cuda")[:, None]
           + torch.arange(BN_VEC, device="cuda")[None, :]) % pat.numel()
    res[:, :BN_VEC] = pat[idx].to(dtype)
    y4, sm, sr, mask = ext.bn_fwd_train_mask(_nhwc(x), w, b, rm, rv,
                                             _nhwc(res), EPS, 0.1, True, None)
    y = _flat(y4)
    assert torch.equal(_unpack(mask, C), y > 0)
    z = y[:, :BN_VEC]
    assert torch.equal(z > 0, res[:, :BN_VEC] > 0)
    assert torch.equal(z, res[:, :BN_VEC].clamp_min(0))  # -0.0 == 0.0
    assert int((z == 0).sum()) == M * BN_VEC * 6 // 8
    out_y = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4, sm, sr, w, True, True, None)
    out_m = ext.bn_bwd_mask(_nhwc(x), _nhwc(dy), mask, sm, sr, w, True, True,
                            None)
    for a, c in zip(out_y, out_m):
        assert torch.equal(a, c)
    # dres = dz: zero wherever y is zero
    assert torch.equal(_flat(out_m[3]) != 0, (y > 0) & (dy != 0))


@pytest.mark.parametrize("need_dres", [False, True], ids=["nodres", "dres"])
@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("C,M", SHAPES, ids=[f"C{c}-M{m}" for c, m in SHAPES])
def test_bwd_mask_equals_bwd_y(ext, C, M, dtype, residual, need_dres):
    f = _forward(C, M, dtype, residual)
    x4, dy4 = _nhwc(f["x"]), _nhwc(f["dy"])
    ws_y, ws_m = _make_ws(C, "persistent")[1], _make_ws(C, "persistent")[1]
    out_y = ext.bn_bwd(x4, dy4, f["y4"], f["sm"], f["sr"], f["w"], True,
                       need_dres, ws_y)
    out_m = ext.bn_bwd_mask(x4, dy4, f["mask"], f["sm"], f["sr"], f["w"],
                            True, need_dres, ws_m)
    assert len(out_y) == len(out_m) == (4 if need_dres else 3)
    for name, a, c in zip(("dx", "dweight", "dbias", "dres"), out_y, out_m):
        assert torch.equal(a, c), name


# ------------------------------------------------------------ unroll tails
def _thread_rows(C, M):
    """Rows each live thread of a streaming reduce adds, as a set. Mirror of
    the kernels' loop: thread (block bx < gm, ty < rows_per_blk) takes rows
    bx * rpb + ty, + gm * rpb, ... below M. With U = BN_RED_U a thread with n
    rows makes n // U unrolled trips and n % U tail trips."""
    g = _geom(C, M)
    first = torch.arange(g["gm"] * g["rpb"])
    stride = g["gm"] * g["rpb"]
    n = torch.where(first < M, (M - 1 - first) // stride + 1,
                    torch.zeros_like(first))
    return set(n.tolist())


def _lane_rows(gm):
    """Partial rows each of the 4 finalize lanes adds: lane ty takes rows
    ty, ty + 4, ... below gm. With U = BN_FIN_U: n // U trips, n % U tail."""
    return [len(range(ty, gm, FIN_LANES)) for ty in range(FIN_LANES)]


def _tail_cases(U):
    """(C, M, per-thread row counts the shape must produce, gm it must give).
    C = 2048 has one row per block (rpb = 1) and gm = 64 for 64 <= M <= 2048,
    so M = 64 k + 1 gives block 0 k + 1 rows and every other block k;
    C = 64 has rpb = 32, so M = 32 * (64 U) + 5 gives rows = 64 U + 1 with
    only 5 live threads in the last one: U + 1 rows for those, U elsewhere.
    gm = ceil(rows / 32) clamped to [64, 512] and to rows."""
    return [
        (8, 3, {0, 1}, 1),                       # rpb 256: ty >= 3 idle
        (8, 257, {0, 1}, 2),
        (2048, 37, {1}, 37),
        (2048, 64 * (U - 1) + 1, {U - 1, U}, 64),
        (2048, 64 * U + 1, {U, U + 1}, 64),
        (2048, 64 * 2 * U + 1, {2 * U, 2 * U + 1}, 64),
        (64, 32 * 64 * U + 5, {U, U + 1}, 64),
        (2048, 3000, {31, 32}, 94),              # 3000 = 94 * 31 + 86
        (2048, 32 * 511 + 1, {31, 32}, GM_MAX),  # smallest M with gm = 512
    ]


def test_tail_cases_cover_the_unroll(ext):
    U, FU = ext.BN_RED_U, ext.BN_FIN_U
    assert U >= 2 and FU >= 2
    seen, lanes = set(), []
    for C, M, rows, gm in _tail_cases(U):
        assert _geom(C, M)["gm"] == gm, (C, M, _geom(C, M))
        assert _thread_rows(C, M) == rows, (C, M, _thread_rows(C, M))
        seen |= rows
        lanes += _lane_rows(gm)
    assert {0, 1, U - 1, U, U + 1, 2 * U + 1} <= seen
    assert {1, 2, 37, 64, 94, 512} <= {c[3] for c in _tail_cases(U)}
    # finalize lanes: idle, one row, tail only, whole trips only, trips with
    # the shortest and the longest tail
    assert 0 in lanes and 1 in lanes
    assert any(0 < n < FU for n in lanes)
    assert any(n >= FU and n % FU == 0 for n in lanes)
    assert any(n > FU and n % FU == 1 for n in lanes)
    assert any(n > FU and n % FU == FU - 1 for n in lanes)


@pytest.mark.parametrize("case", range(len(_tail_cases(4))))
def test_unroll_tails_exact_sums(ext, case):
    """Integer x and dy: every fp32 partial sum is exact (|x| <= 3, |dy| <= 4,
    M < 2^19), so save_mean is the correctly rounded sum / M (fp32 division
    of two exact values; float64 division rounded to fp32 gives the same,
    53 >= 2 * 24 + 2) and dbias is the integer column sum of dz, through the
    y path and through the mask path."""
    C, M, _, _ = _tail_cases(ext.BN_RED_U)[case]
    g = torch.Generator(device="cuda").manual_seed(1000 + case)
    ri = lambda lo, hi: torch.randint(lo, hi, (M, C), generator=g,  # noqa
                                      device="cuda").to(torch.bfloat16)
    x, res, dy = ri(-3, 4), ri(-2, 3), ri(-4, 5)
    w = torch.rand(C, generator=g, device="cuda") + 0.5
    b = torch.randn(C, generator=g, device="cuda")
    rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
    ws_f, ws_b = _make_ws(C, "persistent")
    y4, sm, sr, mask = ext.bn_fwd_train_mask(_nhwc(x), w, b, rm, rv,
                                             _nhwc(res), EPS, 0.1, True, ws_f)
    assert torch.equal(sm, (x.sum(0, dtype=torch.float64) / M).float())
    pos = _flat(y4) > 0
    assert torch.equal(_unpack(mask, C), pos)
    dbias = (dy.float() * pos).sum(0, dtype=torch.float64)
    assert dbias.abs().max().item() < 2 ** 24
    out_y = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4, sm, sr, w, True, True, ws_b)
    assert torch.equal(out_y[2], dbias.float()), "y path"
    out_y = [t.clone() for t in out_y]
    out_m = ext.bn_bwd_mask(_nhwc(x), _nhwc(dy), mask, sm, sr, w, True, True,
                            ws_b)
    assert torch.equal(out_m[2], dbias.float()), "mask path"
    for a, c in zip(out_y, out_m):
        assert torch.equal(a, c)


# ------------------------------------------------------------------ wrapper
@pytest.mark.parametrize("residual", [False, True], ids=["nores", "res"])
def test_wrapper_uses_the_mask_and_repeats_the_y_path(ext, residual):
    from autodist_amd.ops.fused_bn import fused_bn_train
    C, M = 48, 1000
    x, res, dy, w, b, rm, rv = _inputs(C, M, torch.bfloat16, residual, 13)
    rm1, rv1 = rm.clone(), rv.clone()
    r4 = _nhwc(res) if residual else None
    y4, sm, sr = ext.bn_fwd_train(_nhwc(x), w, b, rm, rv, r4, EPS, 0.1, True,
                                  None)
    out = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4, sm, sr, w, True, residual, None)
    xa = _nhwc(x).detach().requires_grad_(True)
    ra = r4.detach().requires_grad_(True) if residual else None
    wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ya = fused_bn_train(xa, wa, ba, rm1, rv1, momentum=0.1, eps=EPS,
                        relu=True, residual=ra, ws=_make_ws(C, "persistent"))
    saved = ya.grad_fn.saved_tensors[1]
    assert saved.dtype == torch.uint8 and saved.shape == (M, C // BN_VEC)
    ya.backward(_nhwc(dy))
    assert torch.equal(ya, y4)
    assert torch.equal(rm1, rm) and torch.equal(rv1, rv)
    assert torch.equal(xa.grad, out[0]) and torch.equal(wa.grad, out[1])
    assert torch.equal(ba.grad, out[2])
    if residual:
        assert torch.equal(ra.grad, out[3])


def test_module_twice_each_backward_has_its_own_mask(ext):
    """One module, two forwards on one workspace, then backward: the masks
    are fresh allocations outside the workspace, and each call's gradient
    is what the direct y-path calls give for that call."""
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d
    bn = FusedBatchNorm2d(16, relu=True).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    xs, gs = _two_inputs()
    rm, rv = bn.running_mean.clone(), bn.running_var.clone()
    w, b = bn.weight.detach().clone(), bn.bias.detach().clone()
    direct = []
    for x, g in zip(xs, gs):
        y4, sm, sr = ext.bn_fwd_train(x.detach(), w, b, rm, rv, None, bn.eps,
                                      bn.momentum, True, None)
        direct.append((y4, ext.bn_bwd(x.detach(), g, y4, sm, sr, w, True,
                                      False, None)))
    ys = [bn(xs[0]), bn(xs[1])]
    masks = [y.grad_fn.saved_tensors[1] for y in ys]
    assert all(m.dtype == torch.uint8 for m in masks)
    assert masks[0].data_ptr() != masks[1].data_ptr()
    assert not torch.equal(masks[0], masks[1])
    for m in masks:
        for t in bn._ws:
            lo = t.data_ptr()
            assert not lo <= m.data_ptr() < lo + t.numel() * t.element_size()
    torch.autograd.backward(ys, gs)
    for i in range(2):
        assert torch.equal(ys[i], direct[i][0])
        assert torch.equal(xs[i].grad, direct[i][1][0])
    # fp32 a + b is commutative: the order of the two backwards is free
    assert torch.equal(bn.weight.grad, direct[0][1][1] + direct[1][1][1])
    assert torch.equal(bn.bias.grad, direct[0][1][2] + direct[1][1][2])
    assert torch.equal(bn.running_mean, rm)
    assert torch.equal(bn.running_var, rv)
