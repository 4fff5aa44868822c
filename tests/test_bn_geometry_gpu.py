"""Fused NHWC BatchNorm kernels across their launch geometries.

tests/test_gpu_kernels.py checks the BN kernels at two shapes that share the
simplest geometry (power-of-two tx_count, grid_c = 1, no grid-stride loop).
Here every row of ROWS forces one branch of the launch maths in
csrc/ext.hip (bn_geom / bn_reduce_gm / bn_grid_m), and the kernels are
called directly (ext.bn_fwd_train / ext.bn_bwd) against a float64 reference
computed from the same quantised inputs.

Error model (nothing here is fitted to what the kernels return):
  * dy holds small integers, so dz = relu-masked dy and every fp32 partial
    sum of it are exact: dbias must be torch.equal to the integer column
    sum, and a dropped or double-counted row fails outright.
  * elementwise outputs stored in bf16 (y, dx, dres): 2^-7 * B + 1e-6, B the
    elementwise sum of |terms| of the reference expression (two bf16 ulps);
    stored in fp32: 2^-20 * B + 1e-6.
  * fp32 reductions (mean, E[x^2], dweight, running stats):
    L * 2^-24 * sum|terms|, L the longest chain of sequential fp32 adds for
    the geometry (see _geom), plus what that error does to values derived
    from the reduction.
The ReLU mask of the reference is the kernel's own y > 0, and the backward
reference takes the kernel's save_mean / save_rstd (they are inputs of
bn_bwd), so bf16 boundary flips and forward error stay out of the sums.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

BN_VEC, BLOCK, GM_MAX, FIN_LANES = 8, 256, 512, 4
EPS = 1e-5


@pytest.fixture(scope="module")
def ext():
    from autodist_amd.ops import api
    assert api.has_gpu_ops(), "HIP extension must be built on a GPU box"
    return api.ext()


def _geom(C, M):
    """Mirror of the launch maths in csrc/ext.hip, to state which branch a
    row forces and to read the accumulation-chain length L off the kernels:
      reduce kernel: each thread adds ceil(rows / gm) rows in its
        grid-stride loop, then the ty == 0 thread adds rows_per_blk - 1 LDS
        partials one after the other;
      finalize kernel: each of the 4 lanes adds ceil(gm / 4) partial rows,
        lane 0 adds the other 3.
    """
    tx = min(C // BN_VEC, BLOCK)
    rpb = BLOCK // tx
    grid_c = -(-(C // BN_VEC) // tx)
    rows = -(-M // rpb)
    gm = min(max(-(-rows // 32), 64), GM_MAX, rows)
    apply_blocks = min(rows, max(4096 // grid_c, 1))
    L = -(-rows // gm) + rpb + -(-gm // FIN_LANES) + FIN_LANES
    assert L <= 1024
    return dict(tx=tx, rpb=rpb, grid_c=grid_c, rows=rows, gm=gm,
                apply_blocks=apply_blocks, leftover=BLOCK - tx * rpb, L=L)


# (C, M, what the geometry must look like) -- one branch per row
ROWS = [
    # tx_count = 1, rows_per_blk = 256, M smaller than one block
    (8, 2, lambda g: g["tx"] == 1 and g["rpb"] == 256 and g["rows"] == 1),
    # same, odd M
    (8, 3, lambda g: g["tx"] == 1 and g["rows"] == 1),
    # ragged second block: one row in block 1
    (8, 257, lambda g: g["tx"] == 1 and g["rows"] == 2),
    # tx_count = 3 does not divide 256: one leftover thread (ty == 85)
    (24, 1000, lambda g: g["tx"] == 3 and g["leftover"] == 1),
    # tx_count = 6: four leftover threads
    (48, 1000, lambda g: g["tx"] == 6 and g["leftover"] == 4),
    # tx_count = 10: six leftover threads
    (80, 1000, lambda g: g["tx"] == 10 and g["leftover"] == 6),
    # reduce grid-stride loop (rows = 193 > gm = 64) with a ragged tail
    (64, 6149, lambda g: g["rows"] == 193 and g["gm"] == 64),
    # tx_count = 256, rows_per_blk = 1, gm floor of 64 with looping
    (2048, 200, lambda g: g["tx"] == 256 and g["rpb"] == 1
        and g["gm"] == 64 and g["rows"] > g["gm"]),
    # grid_c = 2 with one live thread column in the second block
    (2056, 70, lambda g: g["grid_c"] == 2),
    # grid_c = 2, apply grid capped at 2048 < rows
    (4096, 2100, lambda g: g["grid_c"] == 2
        and g["apply_blocks"] == 2048 < g["rows"]),
]
# BN_GM_MAX cap (rows > 16384) and apply cap 4096; ~34M elements: one case
BIG_ROW = (2048, 16500, lambda g: g["gm"] == GM_MAX
           and g["apply_blocks"] == 4096 < g["rows"])


def _nhwc(t2d):
    """[M, C] row-major -> logical [1, C, M, 1], channels_last contiguous."""
    M, C = t2d.shape
    return t2d.view(1, M, 1, C).permute(0, 3, 1, 2)


def _flat(t4d):
    return t4d.permute(0, 2, 3, 1).reshape(-1, t4d.size(1))


def _make_ws(C, mode):
    if mode is None:
        return None, None
    # NaN-filled: whatever a previous call left in the workspace must not
    # reach any output
    return (torch.full((2 * GM_MAX + 4, C), float("nan"), device="cuda"),
            torch.full((2 * GM_MAX + 3, C), float("nan"), device="cuda"))


def _inputs(C, M, dtype, residual, seed, x_mean=0.0, x_std=1.0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    x = (rnd(M, C) * x_std + x_mean).to(dtype)
    res = rnd(M, C).to(dtype) if residual else None
    dy = torch.randint(-4, 5, (M, C), generator=g, device="cuda").to(dtype)
    w = torch.rand(C, generator=g, device="cuda") + 0.5
    b = rnd(C)
    rm = rnd(C)
    rv = torch.rand(C, generator=g, device="cuda") + 0.5
    return x, res, dy, w, b, rm, rv


def _ulp(dtype):
    return 2.0 ** -7 if dtype == torch.bfloat16 else 2.0 ** -20


def _assert_within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    tol = tol.expand_as(err)
    bad = ~(err <= tol)  # NaN counts as outside
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound; worst "
        f"err {err[bad].max().item():.3e} at tol "
        f"{tol[bad][err[bad].argmax()].item():.3e}; max err/tol "
        f"{(err / tol).max().item():.3f}")


def _check_forward(geo, x, res, w, b, rm0, rv0, momentum, relu, y, save_mean,
                   save_rstd, rm, rv, eps=EPS):
    """x, res, y: [M, C]; statistics and their bounds in float64."""
    M = x.size(0)
    L = geo["L"] + 4  # + division, the two products and the subtraction
    xd = x.double()
    mean = xd.mean(0)
    ex2 = (xd * xd).mean(0)
    var = (ex2 - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    u24 = 2.0 ** -24
    tol_mean = L * u24 * xd.abs().mean(0) + 1e-30
    # var = E[x^2] - mean^2, both carried in fp32
    tol_var = L * u24 * (ex2 + 2 * mean.abs() * xd.abs().mean(0)) + 1e-30
    # d rstd / d var = -rstd^3 / 2; rsqrtf itself is good to 2 ulp
    tol_rstd = 0.5 * rstd ** 3 * tol_var + 4 * u24 * rstd
    _assert_within("save_mean", save_mean, mean, tol_mean)
    _assert_within("save_rstd", save_rstd, rstd, tol_rstd)
    wd, bd = w.double(), b.double()
    sc = wd * rstd
    y_ref = xd * sc + (bd - mean * sc)
    B = (xd * sc).abs() + (mean * sc).abs() + bd.abs()
    if res is not None:
        y_ref = y_ref + res.double()
        B = B + res.double().abs()
    if relu:
        y_ref = y_ref.clamp_min(0)  # 1-Lipschitz: the bound carries over
    tol_y = (_ulp(y.dtype) * B + 1e-6 + sc.abs() * tol_mean
             + (xd - mean).abs() * wd.abs() * tol_rstd)
    _assert_within("y", y, y_ref, tol_y)
    if momentum == 0.0:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0), \
            "momentum = 0 must leave the running statistics bit-identical"
        return
    unbias = M / (M - 1) if M > 1 else 1.0
    rm_ref = (1 - momentum) * rm0.double() + momentum * mean
    rv_ref = (1 - momentum) * rv0.double() + momentum * var * unbias
    _assert_within("running_mean", rm, rm_ref, momentum * tol_mean + 4 * u24 * (
        rm0.double().abs() + mean.abs()))
    _assert_within("running_var", rv, rv_ref,
                   momentum * unbias * tol_var + 4 * u24 * (
                       rv0.double().abs() + var * unbias))


def _check_backward(geo, x, dy, y, save_mean, save_rstd, w, relu, dx, dweight,
                    dbias, dres):
    M = x.size(0)
    L = geo["L"] + 4  # + the three roundings inside each term
    u24 = 2.0 ** -24
    dz = dy.double()
    if relu:
        dz = dz * (y > 0)
    # exact: integers, every partial sum below 2^24
    assert dz.abs().sum(0).max().item() < 2 ** 24
    assert torch.equal(dbias, dz.sum(0).float()), \
        f"dbias off by up to {(dbias.double() - dz.sum(0)).abs().max().item()}"
    if dres is not None:
        assert torch.equal(dres, dz.to(dres.dtype)), "dres != dz"
    sm, sr, wd = save_mean.double(), save_rstd.double(), w.double()
    xh = (x.double() - sm) * sr
    terms = dz * xh
    sdzxh = terms.sum(0)
    tol_dw = L * u24 * terms.abs().sum(0) + 1e-30
    _assert_within("dweight", dweight, sdzxh, tol_dw)
    k1, k2, k3 = wd * sr, dz.sum(0) / M, sdzxh / M
    dx_ref = k1 * (dz - k2 - xh * k3)
    B = k1.abs() * (dz.abs() + k2.abs() + (xh * k3).abs())
    tol_dx = _ulp(dx.dtype) * B + 1e-6 + k1.abs() * xh.abs() * tol_dw / M
    _assert_within("dx", dx, dx_ref, tol_dx)


def _run(ext, C, M, dtype, relu, residual, ws_mode=None, momentum=0.1,
         seed=0, **xkw):
    geo = _geom(C, M)
    x, res, dy, w, b, rm, rv = _inputs(C, M, dtype, residual, seed, **xkw)
    rm0, rv0 = rm.clone(), rv.clone()
    ws_f, ws_b = _make_ws(C, ws_mode)
    y4, save_mean, save_rstd = ext.bn_fwd_train(
        _nhwc(x), w, b, rm, rv, _nhwc(res) if residual else None, EPS,
        momentum, relu, ws_f)
    y = _flat(y4)
    _check_forward(geo, x, res, w, b, rm0, rv0, momentum, relu, y, save_mean,
                   save_rstd, rm, rv)
    out = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4, save_mean, save_rstd, w, relu,
                     residual, ws_b)
    dres = _flat(out[3]) if residual else None
    _check_backward(geo, x, dy, y, save_mean, save_rstd, w, relu,
                    _flat(out[0]), out[1], out[2], dres)
    if ws_mode is not None:
        # a second call on the same, now dirty, workspace: the kernels are
        # atomic-free, so every output must repeat bit for bit
        rm2, rv2 = rm0.clone(), rv0.clone()
        y4b, sm2, sr2 = ext.bn_fwd_train(
            _nhwc(x), w, b, rm2, rv2, _nhwc(res) if residual else None, EPS,
            momentum, relu, ws_f)
        out2 = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4b, sm2, sr2, w, relu,
                          residual, ws_b)
        assert torch.equal(y4b, y4) and torch.equal(sm2, save_mean)
        assert torch.equal(sr2, save_rstd) and torch.equal(rm2, rm)
        for a, c in zip(out, out2):
            assert torch.equal(a, c)
        # and the statistics of the first call are still its own
        assert sm2.data_ptr() != save_mean.data_ptr()
    return geo


@pytest.mark.parametrize("relu_res", [True, False], ids=["relu+res", "plain"])
@pytest.mark.parametrize("C,M,forces", ROWS,
                         ids=[f"C{c}-M{m}" for c, m, _ in ROWS])
def test_bn_geometry_row(ext, C, M, forces, relu_res):
    geo = _geom(C, M)
    assert forces(geo), f"row no longer forces its branch: {geo}"
    _run(ext, C, M, torch.bfloat16, relu_res, relu_res, seed=C + M)


def test_bn_geometry_gm_cap(ext):
    C, M, forces = BIG_ROW
    assert forces(_geom(C, M))
    _run(ext, C, M, torch.bfloat16, True, True, seed=1)


@pytest.mark.parametrize("ws_mode", [None, "persistent"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32],
                         ids=["bf16", "fp32"])
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C,M", [(8, 257), (24, 1000)])
def test_bn_flag_cross(ext, C, M, relu, residual, dtype, ws_mode):
    _run(ext, C, M, dtype, relu, residual, ws_mode=ws_mode, seed=7)


def test_bn_momentum_zero_keeps_running_stats(ext):
    _run(ext, 24, 1000, torch.float32, True, True, momentum=0.0, seed=3)


def test_bn_shifted_narrow_channels(ext):
    """Per-channel mean 4, std 0.25: the one-pass E[x^2] - mean^2 variance
    loses (1 + 16^2) * 2^-23 relative, far inside the reduction bound."""
    for dtype in (torch.float32, torch.bfloat16):
        _run(ext, 24, 1000, dtype, True, True, seed=5, x_mean=4.0,
             x_std=0.25)


def test_bn_single_row_closed_form(ext):
    """M = 1: var = 0 and xhat = 0, so y = relu(bias + res) and running_var
    moves toward 0 (what the CPU fallback in fused_bn.py computes)."""
    C, M = 24, 1
    assert _geom(C, M)["rows"] == 1
    x, res, dy, w, b, rm, rv = _inputs(C, M, torch.float32, True, 11)
    rm0, rv0 = rm.clone(), rv.clone()
    y4, save_mean, save_rstd = ext.bn_fwd_train(
        _nhwc(x), w, b, rm, rv, _nhwc(res), EPS, 0.1, True, None)
    xd, bd, rd = x.double(), b.double(), res.double()
    assert torch.equal(save_mean, x[0])
    # var is 0 up to one rounding of x*x (fused multiply-add or not)
    var_tol = 2.0 ** -23 * (xd[0] ** 2)
    rstd0 = EPS ** -0.5
    _assert_within("save_rstd", save_rstd, torch.full_like(xd[0], rstd0),
                   0.5 * rstd0 ** 3 * var_tol + 2.0 ** -22 * rstd0)
    # y = x*sc + (b - mean*sc) + res with sc = w / sqrt(eps): the two large
    # terms cancel, what is left of them is their fp32 rounding
    sc = w.double() * rstd0
    B = 2 * (xd * sc).abs() + bd.abs() + rd.abs()
    _assert_within("y", _flat(y4), (bd + rd).clamp_min(0),
                   2.0 ** -20 * B + 1e-6)
    _assert_within("running_mean", rm, 0.9 * rm0.double() + 0.1 * xd[0],
                   2.0 ** -22 * (rm0.double().abs() + xd[0].abs()))
    _assert_within("running_var", rv, 0.9 * rv0.double(),
                   2.0 ** -22 * rv0.double() + 0.1 * var_tol)
    assert (rv < rv0).all()
    out = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4, save_mean, save_rstd, w, True,
                     True, None)
    dz = dy.double() * (_flat(y4) > 0)
    assert torch.equal(out[2], dz[0].float())
    assert torch.equal(_flat(out[3]), dz.float())
    # dx = k1 * (dz - dz/1 - xhat * k3) with xhat = 0 exactly
    assert torch.equal(out[1], torch.zeros_like(out[1]))
    assert torch.equal(out[0], torch.zeros_like(out[0]))


def test_fused_bn_train_is_the_same_kernels(ext):
    """Through the autograd wrapper, with a persistent workspace: outputs
    and gradients repeat the direct calls bit for bit (atomic-free
    kernels), so the sweep above covers the wrapper too."""
    from autodist_amd.ops.fused_bn import fused_bn_train
    C, M = 48, 1000
    x, res, dy, w, b, rm, rv = _inputs(C, M, torch.bfloat16, True, 13)
    rm1, rv1 = rm.clone(), rv.clone()
    y4, sm, sr = ext.bn_fwd_train(_nhwc(x), w, b, rm, rv, _nhwc(res), EPS,
                                  0.1, True, None)
    out = ext.bn_bwd(_nhwc(x), _nhwc(dy), y4, sm, sr, w, True, True, None)
    xa = _nhwc(x).detach().requires_grad_(True)
    ra = _nhwc(res).detach().requires_grad_(True)
    wa, ba = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    ya = fused_bn_train(xa, wa, ba, rm1, rv1, momentum=0.1, eps=EPS,
                        relu=True, residual=ra, ws=_make_ws(C, "persistent"))
    ya.backward(_nhwc(dy))
    assert torch.equal(ya, y4)
    assert torch.equal(rm1, rm) and torch.equal(rv1, rv)
    assert torch.equal(xa.grad, out[0]) and torch.equal(wa.grad, out[1])
    assert torch.equal(ba.grad, out[2]) and torch.equal(ra.grad, out[3])


# ------------------------------------------------ one module, two forwards
def _ref_two_calls(xs, gs, ys, w, b, eps):
    """float64 F.batch_norm + ReLU (mask: the kernel's own y > 0) for each
    call, loss = sum_i (y_i * g_i).sum(); returns per-call dx and the
    parameter gradients, with the bounds of the module docstring."""
    wd = w.detach().double().requires_grad_(True)
    bd = b.detach().double().requires_grad_(True)
    xds, loss = [], 0.0
    for x, g, y in zip(xs, gs, ys):
        xd = x.detach().double().requires_grad_(True)
        lin = torch.nn.functional.batch_norm(xd, None, None, wd, bd,
                                             training=True, eps=eps)
        loss = loss + (lin * (y.detach() > 0) * g.double()).sum()
        xds.append(xd)
    loss.backward()
    u24 = 2.0 ** -24
    tol_dx, tol_dw, tol_db = [], 0.0, 0.0
    for x, g, y in zip(xs, gs, ys):
        x2, C = _flat(x.detach()).double(), x.size(1)
        M = x2.size(0)
        L = _geom(C, M)["L"] + 4
        dz = _flat(g).double() * (_flat(y.detach()) > 0)
        mean = x2.mean(0)
        ex2 = (x2 * x2).mean(0)
        var = ex2 - mean * mean
        rstd = (var + eps).rsqrt()
        tol_mean = L * u24 * x2.abs().mean(0)
        tol_var = L * u24 * (ex2 + 2 * mean.abs() * x2.abs().mean(0))
        tol_rstd = 0.5 * rstd ** 3 * tol_var + 4 * u24 * rstd
        xh = (x2 - mean) * rstd
        k1 = w.detach().double() * rstd
        sdz_abs, sdzxh_abs = dz.abs().sum(0), (dz * xh).abs().sum(0)
        k2, k3 = dz.sum(0) / M, (dz * xh).sum(0) / M
        # the kernel's xhat carries its own fp32 mean / rstd
        tol_xh = rstd * tol_mean + (x2 - mean).abs() * tol_rstd
        t_dw = L * u24 * sdzxh_abs + (dz.abs() * tol_xh).sum(0)
        t_db = L * u24 * sdz_abs
        B = k1.abs() * (dz.abs() + k2.abs() + (xh * k3).abs())
        dx_abs = k1.abs() * (dz - k2 - xh * k3).abs()
        t_dx = (2.0 ** -20 * B + 1e-6
                + k1.abs() * (t_db / M + xh.abs() * t_dw / M
                              + k3.abs() * tol_xh)
                + dx_abs / rstd * tol_rstd)
        tol_dx.append(t_dx)
        tol_dw, tol_db = tol_dw + t_dw, tol_db + t_db
    return [xd.grad for xd in xds], wd.grad, bd.grad, tol_dx, tol_dw, tol_db


def _two_inputs():
    g = torch.Generator(device="cuda").manual_seed(21)
    mk = lambda: torch.randn(4, 16, 6, 6, generator=g, device="cuda")  # noqa
    x1, x2 = mk(), mk() * 2 + 3
    xs = [t.contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for t in (x1, x2)]
    gs = [mk().contiguous(memory_format=torch.channels_last)
          for _ in range(2)]
    return xs, gs


def _check_two_calls(xs, gs, ys, w, b, eps):
    (ys[0] * gs[0]).sum().add((ys[1] * gs[1]).sum()).backward()
    dxs, dw, db, tol_dx, tol_dw, tol_db = _ref_two_calls(xs, gs, ys, w, b,
                                                         eps)
    for i in range(2):
        _assert_within(f"x{i + 1}.grad", _flat(xs[i].grad), _flat(dxs[i]),
                       tol_dx[i])
    _assert_within("weight.grad", w.grad, dw, tol_dw)
    _assert_within("bias.grad", b.grad, db, tol_db)


def test_module_called_twice_before_backward(ext):
    """Shared tower / two micro-batches summed into one loss: the first
    call's backward must use the first call's statistics, although both
    calls share the module's persistent workspace."""
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d
    bn = FusedBatchNorm2d(16, relu=True).cuda().train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.normal_()
    xs, gs = _two_inputs()
    ys = [bn(xs[0]), bn(xs[1])]
    _check_two_calls(xs, gs, ys, bn.weight, bn.bias, bn.eps)


def test_fused_bn_train_twice_on_one_workspace(ext):
    from autodist_amd.ops.fused_bn import fused_bn_train
    w = (torch.rand(16, device="cuda") + 0.5).requires_grad_(True)
    b = torch.randn(16, device="cuda").requires_grad_(True)
    rm, rv = torch.zeros(16, device="cuda"), torch.ones(16, device="cuda")
    ws = _make_ws(16, "persistent")
    xs, gs = _two_inputs()
    ys = [fused_bn_train(x, w, b, rm, rv, relu=True, ws=ws) for x in xs]
    _check_two_calls(xs, gs, ys, w, b, EPS)
