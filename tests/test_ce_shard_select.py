"""Selection rule of the sharded vocab-parallel CE on CPU tensors: the
torch chain is chosen and nothing tries to load the HIP extension."""
import socket

import pytest
import torch
import torch.distributed as dist


@pytest.fixture()
def world1_pg(monkeypatch):
    monkeypatch.setenv("AUTODIST_FORCE_COLLECTIVES", "1")
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group(
            "gloo", init_method=f"tcp://127.0.0.1:{port}",
            rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_tensors_take_torch_chain(world1_pg, monkeypatch, dtype):
    from autodist_amd.ops import api
    from autodist_amd.parallel.vocab_parallel import VocabParallelProjection

    def no_load():
        raise AssertionError("CPU tensors must not load the extension")
    monkeypatch.setattr(api, "_load", no_load)
    torch.manual_seed(2)
    proj = VocabParallelProjection(50, 16, rank=0, world_size=1)
    hidden = torch.randn(12, 16, dtype=dtype, requires_grad=True)
    targets = torch.randint(0, 50, (12,))
    loss = proj.loss(hidden, targets)
    assert type(loss.grad_fn).__name__ == "_VocabParallelCEBackward"
    loss.backward()
    ref = torch.nn.functional.cross_entropy(
        hidden.detach().float() @ proj.weight.detach().t()
        + proj.bias.detach(), targets)
    assert abs(loss.item() - ref.item()) < (1e-4 if dtype == torch.float32
                                            else 5e-2)
