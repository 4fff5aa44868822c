"""Owner-routed sparse PS push/pull on a WORLD-1 RCCL process group.

With AUTODIST_FORCE_COLLECTIVES=1 the routed path's all-to-all (push) and
allgatherv (pull) are really enqueued on RCCL, the owner applies through the
fused row-wise HIP kernel with shard-local state, and the result must equal
plain torch.optim training (one rank: the mean over ranks is the identity).
Cross-rank movement is covered on gloo (tests/test_sparse_routing_gloo.py).
"""
import socket

import pytest
import torch
import torch.distributed as dist

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


# three uneven shards of 32 rows: [0,11) [11,22) [22,32). Every destination
# resolves to rank 0: the first is replica 0, unknown devices map to rank 0.
DESTINATIONS = ["127.0.0.1:GPU:0", "10.0.0.9:GPU:5", "elsewhere:CPU:0"]
# duplicates on both sides of every shard boundary; step 1 leaves the middle
# shard (rows 11-21) without rows
STEP_IDS = [[0, 0, 10, 11, 21, 22, 31, 31],
            [0, 10, 10, 22, 31],
            [11, 21, 21, 0, 31, 22]]


def _embedding():
    torch.manual_seed(5)
    emb = torch.nn.Embedding(32, 8, sparse=True)
    with torch.no_grad():  # multiples of 2^-8: the SGD arithmetic is exact
        emb.weight.copy_((emb.weight * 256).round() / 256)
    return emb.cuda()


def _routed_engine(emb, opt):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.proto.strategy_ir import Node, PSSynchronizer
    from autodist_amd.strategy.base import Strategy
    g = GraphItem()
    g.extend_model(emb)
    g.extend_optimizer_info(opt)
    (name,) = list(g.trainable_var_op_to_var)
    strategy = Strategy()
    strategy.node_config = [Node(
        var_name=name, partitioner="3,1",
        part_config=[Node(var_name=f"{name}/part_{i}",
                          ps_synchronizer=PSSynchronizer(
                              reduction_destination=d,
                              sparse_routing="owner"))
                     for i, d in enumerate(DESTINATIONS)])]
    strategy.graph_config.replicas = ["127.0.0.1:GPU:0"]
    engine = DistributedEngine(g, strategy, rank=0, world_size=1,
                               device=torch.device("cuda", 0)).setup()
    assert engine.collectives_active
    assert engine.stats()["sparse_routed_vars"] == 1
    (plan,) = engine.var_plans
    assert [(sh.slice.start, sh.slice.end, sh.owner_rank)
            for sh in plan.shards] == [(0, 11, 0), (11, 22, 0), (22, 32, 0)]
    return engine


def _coefs():
    gen = torch.Generator().manual_seed(9)
    return [(torch.rand(len(ids), 8, generator=gen) * 2 - 1).cuda()
            for ids in STEP_IDS]


def _train(emb, opt, coefs):
    for ids, coef in zip(STEP_IDS, coefs):
        ids = torch.tensor(ids, device="cuda")
        opt.zero_grad()
        out = emb(ids)
        (out.sum() if coef is None else (out * coef).sum()).backward()
        opt.step()


def test_world1_rccl_routed_sgd_exact(rccl_world1):
    emb_t = _embedding()
    opt_t = torch.optim.SGD(emb_t.parameters(), lr=0.5)
    _train(emb_t, opt_t, [None] * 3)

    emb_e = _embedding()
    opt_e = torch.optim.SGD(emb_e.parameters(), lr=0.5)
    engine = _routed_engine(emb_e, opt_e)
    _train(emb_e, opt_e, [None] * 3)
    engine.drain()
    torch.cuda.synchronize()
    assert engine.stats()["sparse_rows_received_last_step"] == 0
    engine.teardown()
    assert not torch.equal(emb_e.weight[31], _embedding().weight[31])
    assert torch.equal(emb_t.weight, emb_e.weight), \
        (emb_t.weight - emb_e.weight).abs().max()


def test_world1_rccl_routed_adagrad(rccl_world1):
    coefs = _coefs()
    emb_t = _embedding()
    opt_t = torch.optim.Adagrad(emb_t.parameters(), lr=0.1, lr_decay=0.1)
    _train(emb_t, opt_t, coefs)

    emb_e = _embedding()
    opt_e = torch.optim.Adagrad(emb_e.parameters(), lr=0.1, lr_decay=0.1)
    engine = _routed_engine(emb_e, opt_e)
    _train(emb_e, opt_e, coefs)
    engine.drain()
    torch.cuda.synchronize()
    (plan,) = engine.var_plans
    # shard-local state, every shard's step at the global step (the middle
    # shard had an empty step)
    assert [tuple(sh.state["sum"].shape) for sh in plan.shards] == [
        (11, 8), (11, 8), (10, 8)]
    assert [float(sh.state["step"]) for sh in plan.shards] == [3.0, 3.0, 3.0]
    full = engine.consolidated_optimizer_state()[plan.name]
    engine.teardown()
    err = (emb_t.weight - emb_e.weight).abs().max().item()
    print(f"routed Adagrad vs torch.optim.Adagrad: max err {err:.3e}")
    assert err <= 1e-5
    want_sum = opt_t.state[emb_t.weight]["sum"]
    assert torch.allclose(full["sum"], want_sum, atol=1e-5)
