"""Fused bf16 LayerNorm(+residual) kernels vs fp32 torch reference."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture
def ext():
    from autodist_amd.ops import api
    if not api.has_gpu_ops():
        pytest.skip("no GPU ops")
    return api.ext()


@pytest.mark.parametrize("N,H", [(64, 768), (37, 1024), (128, 3072),
                                 (16, 100)])
def test_ln_fwd_bwd_vs_torch(ext, N, H):
    torch.manual_seed(0)
    x = torch.randn(N, H, device="cuda", dtype=torch.bfloat16)
    res = torch.randn_like(x)
    gamma = torch.randn(H, device="cuda") * 0.5 + 1.0
    beta = torch.randn(H, device="cuda") * 0.1
    dy = torch.randn_like(x)
    y, u, mean, rstd = ext.ln_fwd(x, res, gamma, beta, 1e-12)
    # fp32 reference on the same bf16-quantized inputs
    xf = (x.float() + res.float()).requires_grad_(True)
    gf = gamma.clone().requires_grad_(True)
    bf = beta.clone().requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xf, (H,), gf, bf, 1e-12)
    yr.backward(dy.float())
    assert (y.float() - yr.detach()).abs().max().item() < 3e-2
    # u is stored bf16: allow bf16 quantization of the fp32 sum
    assert torch.allclose(u.float(), x.float() + res.float(), atol=1e-2,
                          rtol=1e-2)
    dx, dgamma, dbeta = ext.ln_bwd(dy, u, gamma, mean, rstd)
    assert (dx.float() - xf.grad).abs().max().item() < 3e-2, \
        (dx.float() - xf.grad).abs().max()
    # column sums over bf16 inputs: looser tol, relative to magnitude
    assert (dgamma - gf.grad).abs().max().item() < \
        0.02 * gf.grad.abs().max().item() + 0.05
    assert (dbeta - bf.grad).abs().max().item() < \
        0.02 * bf.grad.abs().max().item() + 0.05


def test_fused_ln_module_autograd():
    from autodist_amd.ops.fused_ln import FusedLayerNorm
    torch.manual_seed(1)
    H = 768
    m = FusedLayerNorm(H).cuda()
    x = torch.randn(8, 16, H, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    r = torch.randn_like(x, requires_grad=True)
    y = m(x, residual=r)
    assert y.dtype == torch.bfloat16
    y.float().pow(2).mean().backward()
    assert x.grad is not None and r.grad is not None
    assert torch.equal(x.grad, r.grad)  # identity residual gradient
    assert m.weight.grad is not None and m.weight.grad.dtype == torch.float32
    # reference
    xf = (x.detach().float() + r.detach().float()).requires_grad_(True)
    yr = torch.nn.functional.layer_norm(xf, (H,), m.weight.detach(),
                                        m.bias.detach(), m.eps)
    yr.pow(2).mean().backward()
    assert (x.grad.float() - xf.grad).abs().max().item() < 2e-2


def test_bert_layer_fused_ln_trains():
    """BERT layer with fused LN under autocast: bf16 stream, finite grads,
    close to the fp32 reference layer."""
    from autodist_amd.models.bert import BertConfig, BertLayer
    torch.manual_seed(2)
    cfg = BertConfig(hidden=256, heads=4, intermediate=512, dropout=0.0)
    layer = BertLayer(cfg).cuda()
    x = torch.randn(4, 64, 256, device="cuda")
    with torch.autocast("cuda", torch.bfloat16):
        out = layer(x)
    assert out.dtype == torch.bfloat16
    out.float().pow(2).mean().backward()
    for p in layer.parameters():
        assert p.grad is None or torch.isfinite(p.grad.float()).all()


def test_col_sum_and_fused_linear():
    from autodist_amd.ops import api
    torch.manual_seed(5)
    dy = torch.randn(4096, 768, device="cuda", dtype=torch.bfloat16)
    ref = dy.float().sum(0)
    got = api.ext().col_sum(dy)
    assert (got - ref).abs().max().item() < 0.05 * ref.abs().max().item() + 0.1
    # FusedLinear fwd+bwd vs nn.Linear under autocast
    from autodist_amd.ops.fused_linear import FusedLinear
    lin_ref = torch.nn.Linear(768, 512).cuda()
    lin = FusedLinear(768, 512).cuda()
    with torch.no_grad():
        lin.weight.copy_(lin_ref.weight)
        lin.bias.copy_(lin_ref.bias)
    x = torch.randn(8, 32, 768, device="cuda")
    xr = x.clone().requires_grad_(True)
    xf = x.clone().requires_grad_(True)
    with torch.autocast("cuda", torch.bfloat16):
        yr = lin_ref(xr)
        yf = lin(xf)
    assert torch.allclose(yr, yf, atol=2e-2, rtol=1e-2)
    g = torch.randn_like(yr)
    yr.backward(g)
    yf.backward(g)
    assert lin_ref.weight.grad.dtype == lin.weight.grad.dtype
    assert (lin.weight.grad - lin_ref.weight.grad).abs().max().item() < 0.2
    assert (lin.bias.grad - lin_ref.bias.grad).abs().max().item() < \
        0.05 * lin_ref.bias.grad.abs().max().item() + 0.2
    assert (xf.grad - xr.grad).abs().max().item() < 0.1


def test_fused_ce_vs_torch():
    """Online-softmax CE kernels vs F.cross_entropy (loss + input grads)."""
    from autodist_amd.parallel.vocab_parallel import _FusedCERows
    torch.manual_seed(6)
    N, V = 512, 4000
    logits = torch.randn(N, V, device="cuda", dtype=torch.bfloat16) * 3
    targets = torch.randint(0, V, (N,), device="cuda")
    lg = logits.clone().requires_grad_(True)
    loss = _FusedCERows.apply(lg, targets).mean()
    loss.backward()
    lr = logits.float().clone().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, targets)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2e-3 * abs(ref.item()) + 1e-3
    err = (lg.grad.float() - lr.grad).abs().max().item()
    assert err < 5e-5, f"dlogits err {err}"  # grads are O(1/N)


# ---------------------------------------------------------------------------
# Geometry and edge cases. Error model, as in tests/test_bn_geometry_gpu.py:
#   * integer-valued dy / inputs make column sums exact in fp32 -> torch.equal
#   * bf16-stored elementwise outputs: 2^-7 * B + 1e-6, B = sum of |terms|
#   * fp32 reductions: L * 2^-24 * sum|terms|, L = sequential adds in the
#     kernel, plus what that error does to values derived from the reduction
# References are float64 on the same bf16 inputs; the backward reference
# takes the kernel's own u / mean / rstd, which are inputs of ln_bwd.
U24 = 2.0 ** -24
BF16 = 2.0 ** -7


def _within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    tol = tol.expand_as(err)
    bad = ~(err <= tol)
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, "
        f"max err/tol {(err / tol).max().item():.3f}, "
        f"max err {err.max().item():.3e}")


def _ln_chain(H):
    # per thread: ceil(H/2 / 256) pair-iterations of 2 adds; then 4 DPP
    # rotate-adds, 2 cross-group shuffles, 3 adds over the 4 waves; + the
    # division and the roundings inside a term
    return 2 * -(-(H // 2) // 256) + 4 + 2 + 3 + 4


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("N,H", [
    (1, 2),        # one pair: one live thread per row
    (300, 100),    # two ln_bwd_gb row-chunks (blockIdx.y = 1), ragged 2nd
    (513, 514),    # three chunks, last one a single row; ragged pair-iter
    (257, 4094),   # ragged LAST pair-iteration of 8
    (5, 4096),     # H = 256 * LN_MAX_PER_THREAD, the register-array limit
])
def test_ln_geometry(ext, N, H, with_res):
    eps = 1e-5
    g = torch.Generator(device="cuda").manual_seed(N * 10007 + H)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    x = rnd(N, H).bfloat16()
    res = rnd(N, H).bfloat16() if with_res else None
    gamma = rnd(H) * 0.5 + 1.0
    beta = rnd(H) * 0.1
    dy = torch.randint(-4, 5, (N, H), generator=g, device="cuda").bfloat16()
    y, u, mean, rstd = ext.ln_fwd(x, res, gamma, beta, eps)
    L = _ln_chain(H)

    # ---- forward: y is computed from the UNROUNDED fp32 sum x + res
    ud = x.double() + (res.double() if with_res else 0.0)
    if with_res:
        assert torch.equal(u, (x.float() + res.float()).bfloat16())
    else:
        assert u.data_ptr() == x.data_ptr() and torch.equal(u, x)
    m_ref = ud.mean(1)
    ex2 = (ud * ud).mean(1)
    var = (ex2 - m_ref * m_ref).clamp_min(0)
    r_ref = (var + eps).rsqrt()
    tol_m = L * U24 * ud.abs().mean(1) + 1e-30
    tol_v = L * U24 * (ex2 + 2 * m_ref.abs() * ud.abs().mean(1)) + 1e-30
    tol_r = 0.5 * r_ref ** 3 * tol_v + 4 * U24 * r_ref
    _within("mean", mean, m_ref, tol_m)
    _within("rstd", rstd, r_ref, tol_r)
    gd, bd = gamma.double(), beta.double()
    cen = ud - m_ref[:, None]
    y_ref = cen * r_ref[:, None] * gd + bd
    B = (ud.abs() + m_ref.abs()[:, None]) * r_ref[:, None] * gd.abs() \
        + bd.abs()
    _within("y", y, y_ref, BF16 * B + 1e-6
            + (r_ref * tol_m)[:, None] * gd.abs()
            + cen.abs() * gd.abs() * tol_r[:, None])

    # ---- backward, from the kernel's own u / mean / rstd
    dx, dgamma, dbeta = ext.ln_bwd(dy, u, gamma, mean, rstd)
    dyd, md, rd = dy.double(), mean.double(), rstd.double()
    xh = (u.double() - md[:, None]) * rd[:, None]
    # exact: integers, |column sum| <= 4 * 513 < 2^24, also across chunks
    assert torch.equal(dbeta, dyd.sum(0).float()), \
        (dbeta.double() - dyd.sum(0)).abs().max()
    # ln_bwd_gb: 64 sequential adds per row-lane of a 256-row chunk, 3 to
    # combine the lanes, then the chunks; + the roundings inside a term
    Lg = 64 + 3 + -(-N // 256) + 4
    _within("dgamma", dgamma, (dyd * xh).sum(0),
            Lg * U24 * (dyd * xh).abs().sum(0) + 1e-30)
    gg = dyd * gd
    c1, c2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    t1 = L * U24 * gg.abs().mean(1, keepdim=True)
    t2 = L * U24 * (gg * xh).abs().mean(1, keepdim=True)
    dx_ref = rd[:, None] * (gg - c1 - xh * c2)
    Bx = rd[:, None] * (gg.abs() + c1.abs() + (xh * c2).abs())
    _within("dx", dx, dx_ref,
            BF16 * Bx + 1e-6 + rd[:, None] * (t1 + xh.abs() * t2))


def test_ln_constant_row(ext):
    """A constant row has var = 0: with eps = 1e-5 it must come out finite
    and equal to beta (xhat = 0). 3.0 * H is exact in fp32, so mean is."""
    N, H = 3, 100
    x = torch.randn(N, H, device="cuda").bfloat16()
    x[1] = 3.0
    gamma = torch.rand(H, device="cuda") + 0.5
    beta = torch.randn(H, device="cuda")
    y, u, mean, rstd = ext.ln_fwd(x, None, gamma, beta, 1e-5)
    assert torch.isfinite(y.float()).all() and torch.isfinite(rstd).all()
    assert mean[1].item() == 3.0
    _within("y[const]", y[1], beta.double(),
            BF16 * beta.double().abs() + 1e-6)
    dy = torch.randint(-4, 5, (N, H), device="cuda").bfloat16()
    dx, dgamma, dbeta = ext.ln_bwd(dy, u, gamma, mean, rstd)
    assert torch.isfinite(dx.float()).all()
    assert torch.isfinite(dgamma).all()


@pytest.mark.parametrize("N,H", [
    (1, 64),        # one row, one column block
    (513, 100),     # ragged column block (H % 64 != 0), ragged 2nd chunk
    (131079, 64),   # nchunks > 256: the re-chunk branch, ragged last chunk
])
def test_col_sum_exact(ext, N, H):
    g = torch.Generator(device="cuda").manual_seed(N + H)
    x = torch.randint(-4, 5, (N, H), generator=g, device="cuda")
    got = ext.col_sum(x.bfloat16())
    # |sum| <= 4 * 131079 < 2^24: every fp32 partial sum is exact
    assert got.shape == (H,)
    assert torch.equal(got.double(), x.sum(0).double()), \
        (got.double() - x.sum(0).double()).abs().max()


@pytest.mark.parametrize("V", [1, 2, 255, 256, 257, 1000])
def test_fused_ce_edges(ext, V):
    """V < 256 leaves idle threads in the tree combine, V % 256 != 0 a
    ragged last stride; large logits, an all-equal row, -inf entries,
    targets at both ends, and a non-uniform upstream gradient."""
    N = 7
    g = torch.Generator(device="cuda").manual_seed(V)
    logits = torch.randn(N, V, generator=g, device="cuda")
    logits = (logits * (80.0 / logits.abs().max())).bfloat16()
    logits[0] = 60.0                       # all equal: loss = ln V
    targets = torch.randint(0, V, (N,), generator=g, device="cuda")
    targets[2], targets[3] = 0, V - 1
    if V > 1:                              # -inf entries, finite target
        logits[1, 1::2] = float("-inf")
        targets[1] = 0
    dloss = torch.tensor([1.0, 0.5, 0.0, -2.0, 3.0, 1.0 / 7, 0.25],
                         device="cuda")
    loss, m, l2s = ext.ce_fwd(logits, targets)
    dlog = ext.ce_bwd(logits, targets, m, l2s, dloss)

    ld = logits.double()
    lsm = torch.log_softmax(ld, dim=1)
    loss_ref = -lsm.gather(1, targets[:, None])[:, 0]
    assert abs(loss_ref[0].item() - math.log(V)) < 1e-12
    row_max = ld.max(1).values.abs()
    _within("loss", loss, loss_ref,
            2.0 ** -20 * (row_max * math.log2(math.e)).clamp_min(1.0))
    d_ref = lsm.exp()
    d_ref[torch.arange(N), targets] -= 1.0
    d_ref = d_ref * dloss.double()[:, None]
    assert torch.isfinite(dlog.float()).all()
    _within("dlogits", dlog, d_ref,
            BF16 * d_ref.abs() + 1e-4 * dloss.double().abs()[:, None])
    assert torch.equal(dlog[2], torch.zeros_like(dlog[2]))  # weight 0
