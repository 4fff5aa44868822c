"""Fused dropout + residual + LayerNorm kernels (ln_drop_fwd / ln_drop_bwd)
against float64 references on the same bf16 inputs.

The mask comes from attention_ref.drop_keep, the numpy replica of the shared
counter hash: keep[row, col] = drop_keep(1, 1, S, p, seed)[0, 0, row, col].
Error model of tests/test_fused_ln_gpu.py::test_ln_geometry, chain lengths
recomputed for the lane-group reduction trees (G lanes a row, V vectors a
lane, 256 / G rows a block):
  * bf16-stored outputs: 2^-7 * sum|terms| + 1e-6
  * fp32 reductions: L * 2^-24 * sum|terms|
The backward reference takes the kernel's own u / mean / rstd, its inputs.
"""
import functools
import random

import pytest
import torch

from tests.attention_ref import _rkeep, drop_keep

pytestmark = pytest.mark.gpu
U24, BF16 = 2.0 ** -24, 2.0 ** -7
BWD_GRID_MAX = 512     # LND_BWD_GRID_MAX


@pytest.fixture
def ext():
    from autodist_amd.ops import api
    if not api.has_gpu_ops():
        pytest.skip("no GPU ops")
    return api.ext()


def _within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol.expand_as(err))
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, "
        f"max err/tol {(err / tol).max().item():.3f}")


@functools.lru_cache(maxsize=4)
def _keep(N, H, p, seed):
    return drop_keep(1, 1, max(N, H), p, seed)[0, 0, :N, :H].bool().cuda()


def _chains(N, H):
    """Sequential fp32 adds behind a row sum (L) and a dgamma column (Lg)."""
    H8 = H // 8
    G = 64 if H8 <= 64 else 128 if H8 <= 128 else 256
    V = 2 if H8 > 256 else 1
    rpb = 256 // G
    nrb = -(-N // rpb)
    nb = min(nrb, BWD_GRID_MAX)
    # row: 8 V adds a lane, 4 DPP + 2 shuffle steps, G / 64 - 1 wave sums;
    # + 2 roundings forming u = x * rk + res, + the division and the
    # roundings inside a term (4, as in test_ln_geometry)
    L = 8 * V + 6 + (G // 64 - 1) + 2 + 4
    # column: the rows a block walks, its row groups, then the finalize:
    # an eighth of the partial rows a slice, 7 adds over the 8 slices
    Lg = -(-nrb // nb) + (rpb - 1) + -(-nb // 8) + 7 + 4
    return L, Lg


def _fwd_ref(ud, gamma, beta, eps, L):
    """float64 mean, rstd, y of the fp32 u (given in float64), with bounds."""
    m, ex2 = ud.mean(1), (ud * ud).mean(1)
    r = ((ex2 - m * m).clamp_min(0) + eps).rsqrt()
    tol_m = L * U24 * ud.abs().mean(1) + 1e-30
    tol_v = L * U24 * (ex2 + 2 * m.abs() * ud.abs().mean(1)) + 1e-30
    tol_r = 0.5 * r ** 3 * tol_v + 4 * U24 * r
    gd, bd = gamma.double(), beta.double()
    cen = ud - m[:, None]
    B = (ud.abs() + m.abs()[:, None]) * r[:, None] * gd.abs() + bd.abs()
    tol_y = BF16 * B + 1e-6 + (r * tol_m)[:, None] * gd.abs() \
        + cen.abs() * gd.abs() * tol_r[:, None]
    return m, r, tol_m, tol_r, cen * r[:, None] * gd + bd, tol_y


def _bwd_ref(dy, u, gamma, mean, rstd, L):
    """float64 dU with its bound, xhat and c2 of the backward formulas."""
    dyd, rd = dy.double(), rstd.double()[:, None]
    xh = (u.double() - mean.double()[:, None]) * rd
    gg = dyd * gamma.double()
    c1, c2 = gg.mean(1, keepdim=True), (gg * xh).mean(1, keepdim=True)
    t1 = L * U24 * gg.abs().mean(1, keepdim=True)
    t2 = L * U24 * (gg * xh).abs().mean(1, keepdim=True)
    dU = rd * (gg - c1 - xh * c2)
    tol = BF16 * rd * (gg.abs() + c1.abs() + (xh * c2).abs()) + 1e-6 \
        + rd * (t1 + xh.abs() * t2)
    return dU, tol, xh, c2


@pytest.mark.parametrize("with_res", [True, False], ids=["res", "nores"])
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("N,H", [
    (1, 8),         # one live lane
    (5, 512),       # G = 64 full, ragged last block of 4 rows
    (7, 520),       # G = 128, ragged lane tail
    (37, 768),      # the BERT width
    (3, 2056),      # G = 256: second vector live in one lane only
    (5, 4096),      # two full vectors a lane, the register limit
    (600, 2048),    # 600 row blocks on 512: blocks 0..87 take two trips
])
def test_kernels(ext, N, H, p, with_res):
    eps, seed = 1e-5, 4242 + N + H
    g = torch.Generator(device="cuda").manual_seed(N * 10007 + H)
    rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa: E731
    x = rnd(N, H).bfloat16()
    res = rnd(N, H).bfloat16() if with_res else None
    gamma, beta = rnd(H) * 0.5 + 1.0, rnd(H) * 0.1
    dy = torch.randint(-4, 5, (N, H), generator=g, device="cuda").bfloat16()
    keep, rk = _keep(N, H, p, seed), _rkeep(p)
    sd = (p * (1 - p) / (N * H)) ** 0.5
    assert abs(keep.float().mean().item() - (1 - p)) <= 5 * sd
    L, Lg = _chains(N, H)

    y, u, mean, rstd = ext.ln_drop_fwd(x, res, gamma, beta, eps, p, seed)
    rd64 = res.double() if with_res else torch.zeros_like(x).double()
    ud = x.double() * keep * rk + rd64
    # a dropped element is the residual alone: the mask, bit for bit
    assert torch.equal(u[~keep], rd64.bfloat16()[~keep])
    if p == 0.5:
        assert torch.equal(u, (2 * x.float() * keep + rd64.float()).bfloat16())
    _within("u", u, ud, BF16 * ud.abs() + 1e-6)
    m_ref, r_ref, tol_m, tol_r, y_ref, tol_y = _fwd_ref(ud, gamma, beta,
                                                        eps, L)
    _within("mean", mean, m_ref, tol_m)
    _within("rstd", rstd, r_ref, tol_r)
    _within("y", y, y_ref, tol_y)

    dx, dres, dgamma, dbeta = ext.ln_drop_bwd(dy, u, gamma, mean, rstd, p,
                                              seed)
    dU, tol, xh, _ = _bwd_ref(dy, u, gamma, mean, rstd, L)
    _within("dres", dres, dU, tol)
    _within("dx", dx, dU * keep * rk, tol * rk)
    assert torch.equal(dx[~keep], torch.zeros_like(dx[~keep]))
    if p == 0.5:
        assert torch.equal(dx[keep], (2 * dres.float()).bfloat16()[keep])
    dyd = dy.double()
    # integers, |column sum| <= 4 * 600 < 2^24: exact in any order
    assert torch.equal(dbeta, dyd.sum(0).float())
    _within("dgamma", dgamma, (dyd * xh).sum(0),
            Lg * U24 * (dyd * xh).abs().sum(0) + 1e-30)

    # same seed: the same bits; another seed: another mask
    again = ext.ln_drop_fwd(x, res, gamma, beta, eps, p, seed) \
        + ext.ln_drop_bwd(dy, u, gamma, mean, rstd, p, seed)
    for a, b in zip(again, (y, u, mean, rstd, dx, dres, dgamma, dbeta)):
        assert torch.equal(a, b)
    # (eight elements at p = 0.1 can be all kept under both seeds)
    keep2 = _keep(N, H, p, seed + 1)
    u2 = ext.ln_drop_fwd(x, res, gamma, beta, eps, p, seed + 1)[1]
    assert torch.equal(u2[~keep2], rd64.bfloat16()[~keep2])
    assert N * H == 8 or not torch.equal(keep2, keep)
    assert torch.equal(u2, u) == torch.equal(keep2, keep)


def test_params_in_flat_buffer(ext):
    """gamma / beta as views at an odd offset of a flat parameter buffer (4-byte
    aligned only) take scalar loads: the same bits as the float4 path."""
    N, H, p, seed = 9, 776, 0.1, 5
    g = torch.Generator(device="cuda").manual_seed(11)
    x, res, dy = (torch.randn(N, H, generator=g, device="cuda").bfloat16()
                  for _ in range(3))
    flat = torch.randn(2 * H + 2, generator=g, device="cuda")
    gamma, beta = flat[1:H + 1], flat[H + 1:2 * H + 1]
    assert gamma.data_ptr() % 16 and beta.data_ptr() % 16
    outs, refs = [], []
    for ga, be, dst in ((gamma, beta, outs), (gamma.clone(), beta.clone(),
                                              refs)):
        y, u, mean, rstd = ext.ln_drop_fwd(x, res, ga, be, 1e-5, p, seed)
        dst += [y, u, mean, rstd,
                *ext.ln_drop_bwd(dy, u, ga, mean, rstd, p, seed)]
    for a, b in zip(outs, refs):
        assert torch.equal(a, b)


def test_module(ext, monkeypatch):
    from autodist_amd.ops.fused_ln import FusedLayerNorm
    H, p, eps = 768, 0.1, 1e-5
    g = torch.Generator(device="cuda").manual_seed(7)
    m = FusedLayerNorm(H, eps=eps).cuda().train()
    with torch.no_grad():
        m.weight.copy_(torch.randn(H, generator=g, device="cuda") * 0.5 + 1)
        m.bias.copy_(torch.randn(H, generator=g, device="cuda") * 0.1)
    x = torch.randn(4, 8, H, generator=g, device="cuda").bfloat16()
    r = torch.randn(4, 8, H, generator=g, device="cuda").bfloat16()
    w = torch.randint(-4, 5, (32, H), generator=g, device="cuda").float()
    x.requires_grad_(True), r.requires_grad_(True)
    random.seed(99)
    seed = random.getrandbits(31)
    random.seed(99)
    y = m(x, residual=r, dropout_p=p)
    assert y.dtype == torch.bfloat16 and y.shape == x.shape
    (y.float().view(32, H) * w).sum().backward()

    keep, rk = _keep(32, H, p, seed), _rkeep(p)
    L, Lg = _chains(32, H)
    ud = x.detach().double().view(32, H) * keep * rk \
        + r.detach().double().view(32, H)
    gd = m.weight.detach().double()
    mean, rstd, tol_m, tol_r, y_ref, tol_y = _fwd_ref(
        ud, gd, m.bias.detach(), eps, L)
    _within("y", y.view(32, H), y_ref, tol_y)
    # The kernel's backward reads u rounded to bf16 (half an ulp, 2^-9) and
    # its own fp32 mean / rstd: e_x bounds what these do to xhat, and, to
    # first order, through xhat, c2 and the leading rstd to dU
    dU, tol, xh, c2 = _bwd_ref(w, ud, gd, mean, rstd, L)
    rs = rstd[:, None]
    e_x = 2.0 ** -9 * ud.abs() * rs + rs * tol_m[:, None] \
        + xh.abs() * (tol_r / rstd)[:, None]
    gg = (w.double() * gd).abs()
    tol = tol + rs * (e_x * c2.abs() + xh.abs()
                      * (gg * e_x).mean(1, keepdim=True)) \
        + dU.abs() * (tol_r / rstd)[:, None]
    xg, rg = x.grad.view(32, H), r.grad.view(32, H)
    _within("r.grad", rg, dU, tol)
    _within("x.grad", xg, dU * keep * rk, tol * rk)
    # x.grad and r.grad differ as the mask says
    assert torch.equal(xg[~keep], torch.zeros_like(xg[~keep]))
    assert torch.equal((xg != 0) | (rg == 0), keep | (rg == 0))
    assert torch.equal(m.bias.grad, w.sum(0))
    _within("weight.grad", m.weight.grad, (w.double() * xh).sum(0),
            Lg * U24 * (w.double() * xh).abs().sum(0)
            + (w.double().abs() * e_x).sum(0))

    # inactive: the code path of m(x, residual=r), bit for bit
    with torch.no_grad():
        base = m(x, residual=r)
        assert torch.equal(m(x, residual=r, dropout_p=0.0), base)
        assert torch.equal(m.eval()(x, residual=r, dropout_p=p), base)
        monkeypatch.setenv("AUTODIST_LN_DROPOUT", "torch")
        out = m.train()(x, residual=r, dropout_p=p)
    assert out.dtype == torch.bfloat16 and out.shape == x.shape
    assert not torch.equal(out, base)


def test_bert_layer_wiring(ext):
    """Both dropouts of a layer come from hashes: the forward leaves the
    device generator where it was."""
    from autodist_amd.models.bert import BertConfig, BertLayer
    torch.manual_seed(3)
    layer = BertLayer(BertConfig(hidden=256, heads=4, intermediate=512,
                                 dropout=0.1)).cuda().train()
    x = torch.randn(4, 64, 256, device="cuda")
    before = torch.cuda.get_rng_state()
    with torch.autocast("cuda", torch.bfloat16):
        out = layer(x)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    assert out.dtype == torch.bfloat16
    out.float().pow(2).mean().backward()
    for q in layer.parameters():
        assert q.grad is not None and torch.isfinite(q.grad.float()).all()
