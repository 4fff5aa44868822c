"""Fused BN numerics (CPU fallback path) vs torch reference; the GPU HIP
kernels are checked against the same references in test_gpu_kernels.py."""
import copy

import pytest
import torch

from autodist_amd.ops.fused_bn import FusedBatchNorm2d, fused_bn_train


def test_fused_bn_forward_backward_matches_torch():
    torch.manual_seed(0)
    N, C, H, W = 4, 16, 5, 5
    x = torch.randn(N, C, H, W, requires_grad=True)
    res = torch.randn(N, C, H, W, requires_grad=True)
    w = torch.nn.Parameter(torch.rand(C) + 0.5)
    b = torch.nn.Parameter(torch.randn(C))
    rm, rv = torch.zeros(C), torch.ones(C)

    x2 = x.detach().clone().requires_grad_(True)
    res2 = res.detach().clone().requires_grad_(True)
    w2 = torch.nn.Parameter(w.detach().clone())
    b2 = torch.nn.Parameter(b.detach().clone())
    rm2, rv2 = torch.zeros(C), torch.ones(C)

    y = fused_bn_train(x, w, b, rm, rv, momentum=0.1, eps=1e-5, relu=True,
                       residual=res)
    y_ref = torch.relu(torch.nn.functional.batch_norm(
        x2, rm2, rv2, w2, b2, training=True, momentum=0.1, eps=1e-5) + res2)
    assert torch.allclose(y, y_ref, atol=1e-5)
    assert torch.allclose(rm, rm2, atol=1e-6)
    assert torch.allclose(rv, rv2, atol=1e-5)

    g = torch.randn_like(y)
    y.backward(g)
    y_ref.backward(g)
    assert torch.allclose(x.grad, x2.grad, atol=1e-5)
    assert torch.allclose(res.grad, res2.grad, atol=1e-6)
    assert torch.allclose(w.grad, w2.grad, atol=1e-4)
    assert torch.allclose(b.grad, b2.grad, atol=1e-4)


def test_fused_module_state_dict_compatible():
    m = FusedBatchNorm2d(32, relu=True)
    ref = torch.nn.BatchNorm2d(32)
    assert set(m.state_dict().keys()) == set(ref.state_dict().keys())
    # load torch BN weights into fused module
    ref.weight.data.uniform_(0.5, 1.5)
    ref.bias.data.normal_()
    m.load_state_dict(ref.state_dict())
    assert torch.equal(m.weight, ref.weight)


def test_resnet18_fused_matches_unfused_cpu():
    torch.manual_seed(0)
    from autodist_amd.models.resnet import resnet18
    m_ref = resnet18(num_classes=10, fused=False)
    m_fused = resnet18(num_classes=10, fused=True)
    m_fused.load_state_dict(m_ref.state_dict())
    x = torch.randn(2, 3, 64, 64)
    y_ref = m_ref(x)
    y_fused = m_fused(x)
    assert torch.allclose(y_ref, y_fused, atol=1e-4), \
        (y_ref - y_fused).abs().max()
    loss_r = y_ref.square().mean()
    loss_f = y_fused.square().mean()
    loss_r.backward()
    loss_f.backward()
    for (n1, p1), (n2, p2) in zip(m_ref.named_parameters(),
                                  m_fused.named_parameters()):
        assert torch.allclose(p1.grad, p2.grad, atol=1e-3), \
            f"{n1}: {(p1.grad - p2.grad).abs().max()}"


def _assert_fused_matches_unfused(make, x):
    """fused=True must swap kernels, not the model: same forward output and
    parameter gradients on the fallback path (tolerances of the ResNet-18
    test above). Dropout masks are made equal by reseeding. Parameters are
    paired by order: VGG's unfused variant has separate ReLU modules, so
    its Sequential indices differ."""
    torch.manual_seed(0)
    m_ref = make(fused=False)
    m_fused = make(fused=True)
    p_ref, p_fused = list(m_ref.parameters()), list(m_fused.parameters())
    assert [p.shape for p in p_ref] == [p.shape for p in p_fused]
    with torch.no_grad():
        for a, b in zip(p_ref, p_fused):
            b.copy_(a)
    bn_ref = [m for m in m_ref.modules()
              if isinstance(m, torch.nn.BatchNorm2d)]
    bn_fused = [m for m in m_fused.modules()
                if isinstance(m, FusedBatchNorm2d)]
    assert len(bn_ref) == len(bn_fused) > 0
    for a, b in zip(bn_ref, bn_fused):
        assert (a.eps, a.momentum) == (b.eps, b.momentum)
    torch.manual_seed(1)
    y_ref = m_ref(x)
    torch.manual_seed(1)
    y_fused = m_fused(x)
    assert torch.allclose(y_ref, y_fused, atol=1e-4), \
        (y_ref - y_fused).abs().max()
    y_ref.square().mean().backward()
    y_fused.square().mean().backward()
    names = [n for n, _ in m_ref.named_parameters()]
    for n, a, b in zip(names, p_ref, p_fused):
        assert torch.allclose(a.grad, b.grad, atol=1e-3), \
            f"{n}: {(a.grad - b.grad).abs().max()}"
    for a, b in zip(bn_ref, bn_fused):
        assert torch.allclose(a.running_var, b.running_var, atol=1e-4,
                              rtol=1e-4)


def test_inception_v3_fused_matches_unfused_cpu():
    """Whole model, batch 2, 75x75 (the smallest input the model accepts),
    fp32, tolerances of the ResNet-18 test.

    At this size the last two cells run at 1x1: their BatchNorms normalise
    over TWO values per channel, xhat is a smoothed sign function with slope
    1/sqrt(eps) = 32 at zero, and a rounding difference grows by that factor
    through every BN layer in series (torch's own fp32 model is 2e-2 in the
    output and 4e2 in the gradients away from its float64 copy). The
    tolerances hold only because the fallback path of fused_bn.py runs
    torch's own batch-norm kernels, which makes the two variants agree bit
    for bit. With eps=1e-5 in the fused cells against 1e-3 it fails."""
    from autodist_amd.models.inception import inception_v3
    _assert_fused_matches_unfused(
        lambda fused: inception_v3(num_classes=10, fused=fused),
        torch.randn(2, 3, 75, 75, generator=torch.Generator().manual_seed(3)))


def test_inception_cells_fused_match_unfused_cpu():
    """Every top-level cell of Inception v3, fused vs unfused, fed the SAME
    input (the unfused model's activation), so one cell's rounding is not
    amplified by the next: forward output, input gradient and parameter
    gradients at the ResNet-18 tolerances. 107x107 is the smallest input
    that leaves more than two values per channel in the last cells. With
    the fused cells at eps=1e-5 against 1e-3 this fails at the first cell,
    and it names the cell."""
    from autodist_amd.models.inception import inception_v3
    torch.manual_seed(0)
    m_ref = inception_v3(num_classes=10, fused=False)
    m_fused = inception_v3(num_classes=10, fused=True)
    with torch.no_grad():
        for a, b in zip(m_ref.parameters(), m_fused.parameters()):
            b.copy_(a)
    h = torch.randn(2, 3, 107, 107,
                    generator=torch.Generator().manual_seed(3))
    cells_ref = list(m_ref.stem) + list(m_ref.mixed)
    cells_fused = list(m_fused.stem) + list(m_fused.mixed)
    for i, (c_ref, c_fused) in enumerate(zip(cells_ref, cells_fused)):
        h1 = h.detach().clone().requires_grad_(True)
        h2 = h.detach().clone().requires_grad_(True)
        y1, y2 = c_ref(h1), c_fused(h2)
        assert torch.allclose(y1, y2, atol=1e-4), \
            f"cell {i}: {(y1 - y2).abs().max()}"
        g = torch.randn(y1.shape, generator=torch.Generator().manual_seed(i))
        g = g / g.numel() ** 0.5
        y1.backward(g)
        y2.backward(g)
        assert torch.allclose(h1.grad, h2.grad, atol=1e-3), \
            f"cell {i} dx: {(h1.grad - h2.grad).abs().max()}"
        for (n, a), b in zip(c_ref.named_parameters(),
                             c_fused.parameters()):
            assert torch.allclose(a.grad, b.grad, atol=1e-3), \
                f"cell {i} {n}: {(a.grad - b.grad).abs().max()}"
        h = y1.detach()


def test_vgg16_bn_fused_matches_unfused_cpu():
    from autodist_amd.models.vgg import vgg16
    # 32x32: five 2x2 max-pools leave 1x1
    _assert_fused_matches_unfused(
        lambda fused: vgg16(num_classes=10, batch_norm=True, fused=fused),
        torch.randn(2, 3, 32, 32, generator=torch.Generator().manual_seed(4)))


def test_fused_bn_eval_mode():
    torch.manual_seed(1)
    m = FusedBatchNorm2d(8, relu=False)
    ref = torch.nn.BatchNorm2d(8)
    ref.load_state_dict(m.state_dict())
    x = torch.randn(3, 8, 4, 4)
    m.train()
    ref.train()
    m(x)
    ref(x)
    m.eval()
    ref.eval()
    x2 = torch.randn(3, 8, 4, 4)
    assert torch.allclose(m(x2), ref(x2), atol=1e-5)
