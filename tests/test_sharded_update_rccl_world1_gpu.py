"""The sharded dense schedule on RCCL.

World 1 with AUTODIST_FORCE_COLLECTIVES=1 (see tests/test_rccl_world1_gpu.py
for why this is the deepest single-GPU proof): the real ncclReduceScatter and
ncclAllGather are enqueued on the comm stream, the optimizer kernels consume
the (bf16) wire shard, and the compute stream waits on the gathers. A one-rank
sum is the identity, so the sharded engine must equal the all-reduce engine
bit for bit. Cross-rank movement is covered on gloo
(tests/test_sharded_update_gloo.py) and by the world-2 case below whenever
two GPUs are visible.
"""
import socket

import pytest
import torch
import torch.distributed as dist

from tests.dist_utils import run_distributed

pytestmark = pytest.mark.gpu


@pytest.fixture()
def rccl_world1(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("AUTODIST_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group(
            "nccl", init_method=f"tcp://127.0.0.1:{port}",
            rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


def _mlp(seed, dev="cuda"):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(64, 256), torch.nn.Tanh(),
                               torch.nn.Linear(256, 32)).to(dev)


OPTIMIZERS = {
    "sgdm": lambda ps: torch.optim.SGD(ps, lr=0.05, momentum=0.9),
    "adamw": lambda ps: torch.optim.AdamW(ps, lr=1e-2),
}


def _build_engine(model, opt, schedule, compressor, rank=0, world=1,
                  dev=None):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.resource_spec import ResourceSpec
    from autodist_amd.strategy import AllReduce
    g = GraphItem()
    g.extend_model(model)
    g.extend_optimizer_info(opt)
    strategy = AllReduce(compressor=compressor, schedule=schedule).build(
        g, ResourceSpec())
    if world > 1:
        strategy.graph_config.replicas = [
            f"127.0.0.1:GPU:{r}" for r in range(world)]
    engine = DistributedEngine(g, strategy, rank=rank, world_size=world,
                               device=dev or torch.device("cuda", 0))
    engine.setup()
    assert engine.collectives_active
    return engine


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


@pytest.mark.parametrize("opt_name", ["sgdm", "adamw"])
@pytest.mark.parametrize("compressor", ["NoneCompressor", "HorovodCompressor",
                                        "HorovodCompressorEF"])
def test_world1_rccl_sharded_equals_allreduce(rccl_world1, compressor,
                                              opt_name):
    torch.manual_seed(21)
    data = [(torch.randn(16, 64, device="cuda"),
             torch.randn(16, 32, device="cuda")) for _ in range(4)]
    runs = {}
    for schedule in ("allreduce", "sharded"):
        model = _mlp(3)
        opt = OPTIMIZERS[opt_name](model.parameters())
        engine = _build_engine(model, opt, schedule, compressor)
        for x, y in data:
            opt.zero_grad()
            torch.nn.functional.mse_loss(model(x), y).backward()
            opt.step()
        engine.drain()
        torch.cuda.synchronize()
        runs[schedule] = (model, engine.stats(), engine)
        engine.teardown()
    m_ar, st_ar, _ = runs["allreduce"]
    m_sh, st_sh, e_sh = runs["sharded"]
    for (name, pa), pb in zip(m_ar.named_parameters(), m_sh.parameters()):
        assert torch.equal(_bits(pa), _bits(pb)), \
            f"{name}: {(pa - pb).abs().max().item()}"
    assert not torch.equal(m_sh[0].weight, _mlp(3)[0].weight)  # it trained
    numel = sum(p.numel() for p in m_sh.parameters())
    assert numel % 8 == 0  # no pad at world 1 for this model
    wire_elt = 4 if compressor == "NoneCompressor" else 2
    assert st_sh["sharded_buckets"] == len(e_sh.buckets) > 0
    assert st_sh["reduce_scatter_bytes_per_step"] == numel * wire_elt
    assert st_sh["allgather_bytes_per_step"] == numel * 4
    assert st_sh["allreduce_bytes_per_step"] == 0
    assert st_ar["sharded_buckets"] == 0
    assert st_ar["reduce_scatter_bytes_per_step"] == 0
    assert st_ar["allreduce_bytes_per_step"] == numel * 4
    if compressor != "NoneCompressor":
        # the update consumed the bf16 wire shard, nothing was cast back
        for b in e_sh.buckets:
            assert b.compressor._shard.dtype == torch.bfloat16


# ------------------------------------------------------------ world 2 on GPU
def _world2_case(rank, world):
    dev = torch.device("cuda", rank % torch.cuda.device_count())
    torch.cuda.set_device(dev)
    torch.manual_seed(100 + rank)
    data = [(torch.randn(16, 64, device=dev),
             torch.randn(16, 32, device=dev)) for _ in range(3)]
    models = {}
    for schedule in ("allreduce", "sharded"):
        model = _mlp(3, dev)
        opt = OPTIMIZERS["adamw"](model.parameters())
        engine = _build_engine(model, opt, schedule, "HorovodCompressor",
                               rank=rank, world=world, dev=dev)
        for x, y in data:
            opt.zero_grad()
            torch.nn.functional.mse_loss(model(x), y).backward()
            opt.step()
        engine.drain()
        torch.cuda.synchronize()
        if schedule == "sharded":
            for b in engine.buckets:
                assert b.state["exp_avg"].numel() == b.shard_len
                assert b.shard_len * world == b.padded_numel
        engine.teardown()
        models[schedule] = model
    # a two-term sum has no order: bitwise equal to the all-reduce engine
    for pa, pb in zip(models["allreduce"].parameters(),
                      models["sharded"].parameters()):
        assert torch.equal(_bits(pa), _bits(pb))
        both = [torch.empty_like(pb) for _ in range(world)]
        dist.all_gather(both, pb.detach().contiguous())
        assert torch.equal(_bits(both[0]), _bits(both[1]))


def test_world2_rccl_sharded_equals_allreduce():
    if not torch.cuda.is_available() or torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    run_distributed(_world2_case, world_size=2, backend="nccl", timeout=240)
