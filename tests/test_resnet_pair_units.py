"""The fused ResNet walks its blocks itself and chains them by forward_pair.

On the CPU forward_pair returns the same tensor twice and the BN runs through
torch's own kernels, so the hand-walked fused model must be the unfused model
down to the last bit: output, every parameter gradient, every buffer.
"""
import torch


def _fused_and_ref(make):
    torch.manual_seed(0)
    m_ref = make(num_classes=10, fused=False)
    m_fused = make(num_classes=10, fused=True)
    m_fused.load_state_dict(m_ref.state_dict())
    return m_fused, m_ref


def test_forward_pair_returns_one_tensor_twice_on_cpu():
    from autodist_amd.models.resnet import BasicBlock, Bottleneck
    for cls in (BasicBlock, Bottleneck):
        torch.manual_seed(1)
        block = cls(16 * cls.expansion, 16, fused=True).train()
        x = torch.randn(2, 16 * cls.expansion, 6, 6)
        y_main, y_res = block.forward_pair((x, x))
        assert y_main is y_res
        torch.manual_seed(1)
        twin = cls(16 * cls.expansion, 16, fused=True).train()
        assert torch.equal(twin(x), y_main)
        assert torch.equal(twin.forward_pair((x, x.clone()))[0], y_main)


def test_resnet18_hand_walked_layers_equal_unfused_bitwise():
    from autodist_amd.models.resnet import resnet18
    m_fused, m_ref = _fused_and_ref(resnet18)
    assert list(m_fused.state_dict()) == list(m_ref.state_dict())
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(5))
    y_ref, y_fused = m_ref(x), m_fused(x)
    assert torch.equal(y_ref, y_fused)
    y_ref.square().mean().backward()
    y_fused.square().mean().backward()
    for (n1, p1), (n2, p2) in zip(m_ref.named_parameters(),
                                  m_fused.named_parameters()):
        assert n1 == n2
        assert torch.equal(p1.grad, p2.grad), n1
    for (n1, b1), (n2, b2) in zip(m_ref.named_buffers(),
                                  m_fused.named_buffers()):
        assert n1 == n2
        assert torch.equal(b1, b2), n1


def test_fused_resnet_eval_walks_the_same_blocks():
    from autodist_amd.models.resnet import resnet18
    m_fused, m_ref = _fused_and_ref(resnet18)
    m_fused.eval()
    m_ref.eval()
    x = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(6))
    with torch.no_grad():
        assert torch.allclose(m_fused(x), m_ref(x), atol=1e-4)
