"""Numerics tests for the gfx950 HIP kernels vs plain PyTorch fp32 references.

Every kernel in ops/csrc/*.hip has a test here (run with `-m gpu` on an
MI355X box), at one or two shapes in its simplest launch geometry. The other
branches of the launch maths and the optimizer flags are covered in
test_bn_geometry_gpu.py, test_fused_ln_gpu.py and
test_optimizer_matrix_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ext():
    from autodist_amd.ops import api
    assert api.has_gpu_ops(), "HIP extension must be built on a GPU box"
    return api.ext()


def _rand(n, seed=0, device="cuda"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(n, generator=g, device=device, dtype=torch.float32)


N_SIZES = [1, 63, 257, 1 << 20, (1 << 20) + 3]


@pytest.mark.parametrize("n", N_SIZES)
def test_fused_sgd_plain(ext, n):
    p = _rand(n, 1)
    g = _rand(n, 2)
    p_ref = p.clone()
    ext.fused_sgd(p, g, None, 0.1, 0.0, 0.0, 1e-4, False, False, False)
    ref = p_ref - 0.1 * (g + 1e-4 * p_ref)
    assert torch.allclose(p, ref, atol=1e-6)


@pytest.mark.parametrize("nesterov", [False, True])
def test_fused_sgd_momentum(ext, nesterov):
    n = 100000
    p = _rand(n, 1)
    g1, g2 = _rand(n, 2), _rand(n, 3)
    # reference: torch.optim.SGD on a clone
    p_ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.SGD([p_ref], lr=0.1, momentum=0.9, nesterov=nesterov)
    for gg in (g1, g2):
        p_ref.grad = gg.clone()
        opt.step()
    buf = torch.empty_like(p)
    ext.fused_sgd(p, g1, buf, 0.1, 0.9, 0.0, 0.0, nesterov, True, False)
    ext.fused_sgd(p, g2, buf, 0.1, 0.9, 0.0, 0.0, nesterov, False, False)
    assert torch.allclose(p, p_ref.detach(), atol=1e-6)


@pytest.mark.parametrize("adamw", [False, True])
def test_fused_adam(ext, adamw):
    n = 100000
    p = _rand(n, 1)
    p_ref = torch.nn.Parameter(p.clone())
    cls = torch.optim.AdamW if adamw else torch.optim.Adam
    opt = cls([p_ref], lr=1e-2, weight_decay=0.02)
    m = torch.zeros_like(p)
    v = torch.zeros_like(p)
    for step in range(1, 4):
        g = _rand(n, 10 + step)
        p_ref.grad = g.clone()
        opt.step()
        bc1 = 1 - 0.9 ** step
        sqrt_bc2 = (1 - 0.999 ** step) ** 0.5
        ext.fused_adam(p, g, m, v, 1e-2, 0.9, 0.999, 1e-8, 0.02, adamw,
                       bc1, sqrt_bc2, False)
    assert torch.allclose(p, p_ref.detach(), atol=1e-5), \
        (p - p_ref.detach()).abs().max()


def test_scale_cast_roundtrip(ext):
    n = 1 << 16
    x = _rand(n, 5)
    wire = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    ext.scale_cast_bf16(x, wire, 0.25)
    ref = (x * 0.25).to(torch.bfloat16)
    assert torch.equal(wire, ref)
    back = torch.empty_like(x)
    ext.cast_back_f32(wire, back)
    assert torch.equal(back, ref.to(torch.float32))


def test_ef_compress(ext):
    n = 4097
    flat = _rand(n, 6)
    err = _rand(n, 7) * 0.01
    flat_ref = flat + err
    wire_ref = (flat_ref * 0.5).to(torch.bfloat16)
    err_ref = flat_ref - wire_ref.to(torch.float32) / 0.5
    wire = torch.empty(n, dtype=torch.bfloat16, device="cuda")
    ext.ef_compress(flat, err, wire, 0.5)
    assert torch.equal(wire, wire_ref)
    assert torch.allclose(flat, flat_ref, atol=1e-7)
    assert torch.allclose(err, err_ref, atol=1e-7)


def test_segment_coalesce(ext):
    idx = torch.tensor([5, 1, 5, 3, 1, 1], device="cuda")
    vals = torch.arange(24, device="cuda", dtype=torch.float32).view(6, 4)
    uniq, out = ext.segment_coalesce(idx, vals)
    assert uniq.tolist() == [1, 3, 5]
    ref = torch.zeros(3, 4, device="cuda")
    ref[0] = vals[1] + vals[4] + vals[5]
    ref[1] = vals[3]
    ref[2] = vals[0] + vals[2]
    assert torch.allclose(out, ref)


def test_gather_scatter_rows(ext):
    src = _rand(50 * 8, 3).view(50, 8)
    idx = torch.tensor([0, 7, 49, 7], device="cuda")
    out = ext.gather_rows(src, idx)
    assert torch.allclose(out, src[idx])
    acc = torch.zeros_like(src)
    ext.scatter_add_rows(acc, idx, out)
    ref = torch.zeros_like(src)
    ref.index_add_(0, idx, out)
    assert torch.allclose(acc, ref)


def test_fused_bn_gpu_vs_cpu_reference(ext):
    """HIP fused BN (bf16 NHWC, +add+relu) vs the CPU fp32 torch reference."""
    torch.manual_seed(0)
    N, C, H, W = 8, 64, 14, 14
    x32 = torch.randn(N, C, H, W)
    res32 = torch.randn(N, C, H, W)
    w = torch.rand(C) + 0.5
    b = torch.randn(C)
    # CPU fp32 reference
    rm_c, rv_c = torch.zeros(C), torch.ones(C)
    xc = x32.clone().requires_grad_(True)
    rc = res32.clone().requires_grad_(True)
    wc = torch.nn.Parameter(w.clone())
    bc = torch.nn.Parameter(b.clone())
    z_ref = torch.nn.functional.batch_norm(
        xc, rm_c, rv_c, wc, bc, training=True, momentum=0.1, eps=1e-5) + rc
    y_ref = torch.relu(z_ref)
    gy = torch.randn(N, C, H, W)
    y_ref.backward(gy)
    # GPU bf16 fused
    from autodist_amd.ops.fused_bn import fused_bn_train
    dev = torch.device("cuda")
    xg = x32.to(dev, torch.bfloat16).contiguous(
        memory_format=torch.channels_last).requires_grad_(True)
    rg = res32.to(dev, torch.bfloat16).contiguous(
        memory_format=torch.channels_last).requires_grad_(True)
    wg = torch.nn.Parameter(w.to(dev))
    bg = torch.nn.Parameter(b.to(dev))
    rm_g, rv_g = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    y = fused_bn_train(xg, wg, bg, rm_g, rv_g, momentum=0.1, eps=1e-5,
                       relu=True, residual=rg)
    y.backward(gy.to(dev, torch.bfloat16).contiguous(
        memory_format=torch.channels_last))
    tol = 5e-2  # bf16 inputs vs fp32 reference
    assert torch.allclose(y.detach().float().cpu(), y_ref.detach(), atol=tol)
    assert torch.allclose(rm_g.cpu(), rm_c, atol=1e-2)
    assert torch.allclose(rv_g.cpu(), rv_c, atol=1e-2)
    # Backward: compare against a torch fp32 reference computed from the
    # KERNEL'S saved forward tensors (same mask / same quantized inputs), so
    # relu-boundary bf16 mask flips don't poison summed statistics.
    xq = xg.detach().float().cpu()
    yq = y.detach().float().cpu()
    dyq = gy.to(torch.bfloat16).float()
    mean_q = torch.zeros(C)
    rstd_q = torch.zeros(C)
    # recompute stats exactly like the kernel (fp32 over quantized x)
    mean_q = xq.mean((0, 2, 3))
    var_q = xq.var((0, 2, 3), unbiased=False)
    rstd_q = (var_q + 1e-5).rsqrt()
    dz = dyq * (yq > 0).float()
    M = N * H * W
    xhat = (xq - mean_q[None, :, None, None]) * rstd_q[None, :, None, None]
    sum_dz = dz.sum((0, 2, 3))
    sum_dzxh = (dz * xhat).sum((0, 2, 3))
    dx_ref = (w * rstd_q)[None, :, None, None] * (
        dz - sum_dz[None, :, None, None] / M
        - xhat * sum_dzxh[None, :, None, None] / M)
    assert torch.allclose(xg.grad.float().cpu(), dx_ref, atol=tol), \
        (xg.grad.float().cpu() - dx_ref).abs().max()
    assert torch.allclose(rg.grad.float().cpu(), dz.to(torch.bfloat16).float(),
                          atol=tol)
    assert torch.allclose(wg.grad.cpu(), sum_dzxh, atol=0.3), \
        (wg.grad.cpu() - sum_dzxh).abs().max()
    assert torch.allclose(bg.grad.cpu(), sum_dz, atol=0.3)


def test_fused_bn_gpu_fp32_exact(ext):
    """fp32 path of the HIP BN kernels: tight tolerance vs torch."""
    torch.manual_seed(2)
    N, C, H, W = 4, 32, 7, 7
    dev = torch.device("cuda")
    x32 = torch.randn(N, C, H, W, device=dev)
    w = torch.nn.Parameter(torch.rand(C, device=dev) + 0.5)
    b = torch.nn.Parameter(torch.randn(C, device=dev))
    rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
    from autodist_amd.ops.fused_bn import fused_bn_train
    xg = x32.clone().contiguous(
        memory_format=torch.channels_last).requires_grad_(True)
    y = fused_bn_train(xg, w, b, rm, rv, relu=True)
    gy = torch.randn_like(y)
    y.backward(gy)
    xc = x32.clone().cpu().requires_grad_(True)
    wc = torch.nn.Parameter(w.detach().cpu())
    bc = torch.nn.Parameter(b.detach().cpu())
    rmc, rvc = torch.zeros(C), torch.ones(C)
    yr = torch.relu(torch.nn.functional.batch_norm(
        xc, rmc, rvc, wc, bc, training=True, momentum=0.1, eps=1e-5))
    yr.backward(gy.cpu())
    assert torch.allclose(y.detach().cpu(), yr.detach(), atol=1e-4)
    assert torch.allclose(xg.grad.cpu(), xc.grad, atol=1e-4)
    assert torch.allclose(w.grad.cpu(), wc.grad, atol=1e-2)
    assert torch.allclose(b.grad.cpu(), bc.grad, atol=1e-2)
    assert torch.allclose(rm.cpu(), rmc, atol=1e-5)
    assert torch.allclose(rv.cpu(), rvc, atol=1e-4)


def test_psgd_mfma_gemms(ext):
    """PowerSGD MFMA factor GEMMs vs torch.matmul (rocBLAS) reference."""
    torch.manual_seed(0)
    n, s, r = 192, 256, 4
    M = torch.randn(n, s, device="cuda")
    Qp = torch.zeros(s, 16, device="cuda")
    Qp[:, :r] = torch.randn(s, r, device="cuda")
    P = ext.psgd_mq(M, Qp)
    P_ref = M @ Qp
    assert torch.allclose(P, P_ref, atol=1e-3), (P - P_ref).abs().max()
    Pp = torch.zeros(n, 16, device="cuda")
    Pp[:, :r] = torch.randn(n, r, device="cuda")
    Q2 = ext.psgd_mtp(M, Pp)
    Q2_ref = M.t() @ Pp
    assert torch.allclose(Q2, Q2_ref, atol=1e-3), (Q2 - Q2_ref).abs().max()


def test_psgd_decompress_ef(ext):
    torch.manual_seed(1)
    side = 128
    numel = side * side - 37
    flat = torch.randn(numel, device="cuda")
    err = torch.zeros(numel, device="cuda")
    m_local = torch.randn(side, side, device="cuda")
    Pp = torch.randn(side, 16, device="cuda")
    Qp = torch.randn(side, 16, device="cuda")
    scale = 0.5
    hat_ref = (Pp @ Qp.t()).mul(scale).view(-1)[:numel]
    err_ref = m_local.view(-1)[:numel] - hat_ref
    ext.psgd_decompress_ef(flat, err, m_local, Pp, Qp, scale)
    assert torch.allclose(flat, hat_ref, atol=1e-4)
    assert torch.allclose(err, err_ref, atol=1e-4)


def test_psgd_add_err_pad(ext):
    flat = torch.randn(100, device="cuda")
    err = torch.randn(100, device="cuda")
    out = torch.full((128,), 7.0, device="cuda")
    ext.psgd_add_err_pad(flat, err, out)
    assert torch.allclose(out[:100], flat + err)
    assert (out[100:] == 0).all()


def test_powersgd_compressor_gpu_roundtrip(monkeypatch):
    """End-to-end PowerSGD compressor on GPU (collectives stubbed: world=1)
    — the low-rank projection must match the CPU torch implementation."""
    import torch.distributed as dist
    from autodist_amd.parallel import powersgd as psgd_mod
    monkeypatch.setattr(dist, "all_reduce",
                        lambda *a, **k: None)
    from autodist_amd.parallel.powersgd import PowerSGDCompressor
    torch.manual_seed(5)
    numel = 5000
    flat_gpu = torch.randn(numel, device="cuda")
    flat_cpu = flat_gpu.cpu().clone()
    cg = PowerSGDCompressor("v", rank=4)
    cc = PowerSGDCompressor("v", rank=4)
    for _ in range(3):
        hg = cg.reduce(flat_gpu, group=None, async_op=False, scale=1.0)
        cg.finalize(flat_gpu, hg)
        hc = cc.reduce(flat_cpu, group=None, async_op=False, scale=1.0)
        cc.finalize(flat_cpu, hc)
    assert torch.allclose(flat_gpu.cpu(), flat_cpu, atol=1e-2), \
        (flat_gpu.cpu() - flat_cpu).abs().max()


def test_apply_flat_dispatch_uses_hip():
    """apply_flat on GPU must route through the HIP kernel and match the
    CPU torch reference."""
    from autodist_amd.parallel import apply as apply_mod
    n = 12345
    p_gpu = _rand(n, 1)
    g_gpu = _rand(n, 2)
    p_cpu, g_cpu = p_gpu.cpu(), g_gpu.cpu()
    hyper = {"lr": 0.1, "momentum": 0.9, "dampening": 0.0,
             "weight_decay": 1e-4, "nesterov": True}
    st_gpu, st_cpu = {}, {}
    for _ in range(2):
        apply_mod.apply_flat("SGD", p_gpu, g_gpu, st_gpu, hyper)
        apply_mod.apply_dense("SGD", [p_cpu], [g_cpu], [st_cpu], hyper)
    assert torch.allclose(p_gpu.cpu(), p_cpu, atol=1e-6)


def test_fused_adagrad(ext):
    n = 100000
    p = _rand(n, 2)
    p_ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.Adagrad([p_ref], lr=5e-2, weight_decay=0.01,
                              lr_decay=0.1)
    acc = torch.zeros_like(p)
    for step in range(1, 4):
        g = _rand(n, 20 + step)
        p_ref.grad = g.clone()
        opt.step()
        clr = 5e-2 / (1 + (step - 1) * 0.1)
        ext.fused_adagrad(p, g, acc, clr, 1e-10, 0.01, False)
    assert torch.allclose(p, p_ref.detach(), atol=1e-5), \
        (p - p_ref.detach()).abs().max()


@pytest.mark.parametrize("centered,momentum", [(False, 0.0), (True, 0.9),
                                               (False, 0.9), (True, 0.0)])
def test_fused_rmsprop(ext, centered, momentum):
    n = 65536
    p = _rand(n, 3)
    p_ref = torch.nn.Parameter(p.clone())
    opt = torch.optim.RMSprop([p_ref], lr=1e-3, alpha=0.95, momentum=momentum,
                              centered=centered, weight_decay=0.02)
    sq = torch.zeros_like(p)
    ga = torch.zeros_like(p) if centered else None
    buf = torch.zeros_like(p) if momentum else None
    for step in range(3):
        g = _rand(n, 30 + step)
        p_ref.grad = g.clone()
        opt.step()
        ext.fused_rmsprop(p, g, sq, ga, buf, 1e-3, 0.95, 1e-8, 0.02,
                          momentum, False)
    assert torch.allclose(p, p_ref.detach(), atol=1e-5), \
        (p - p_ref.detach()).abs().max()
