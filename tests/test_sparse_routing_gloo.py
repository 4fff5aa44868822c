"""Owner-routed sparse PS push/pull (gloo, CPU).

A sparse variable on a synchronous PS with sparse_routing="owner" pushes its
locally coalesced rows to the shard owners (all-to-all), the owners apply
them with shard-local optimizer state, and the updated rows are pulled back
(allgatherv). These tests hold that path against the replicated path
(allgather of every rank's raw rows + the full update on every rank), which
computes the same update by construction.
"""
import pytest
import torch

from tests.dist_utils import run_distributed

pytestmark = pytest.mark.integration


def _engine(rank, world, emb, opt, owners, routing, staleness=0):
    """Engine over a hand-built strategy: the embedding table is split into
    len(owners) row shards (torch.tensor_split boundaries), shard i owned by
    rank owners[i]."""
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.proto.strategy_ir import Node, PSSynchronizer
    from autodist_amd.strategy.base import Strategy

    g = GraphItem()
    g.extend_model(emb)
    g.extend_optimizer_info(opt)
    (name,) = list(g.trainable_var_op_to_var)
    replicas = [f"127.0.0.1:CPU:{r}" for r in range(world)]
    parts = [Node(var_name=f"{name}/part_{i}",
                  ps_synchronizer=PSSynchronizer(
                      reduction_destination=replicas[o], staleness=staleness,
                      sparse_routing=routing))
             for i, o in enumerate(owners)]
    strategy = Strategy()
    strategy.node_config = [Node(var_name=name,
                                 partitioner=f"{len(owners)},1",
                                 part_config=parts)]
    strategy.graph_config.replicas = replicas
    engine = DistributedEngine(g, strategy, rank=rank, world_size=world,
                               device=torch.device("cpu")).setup()
    return g, engine


def _gather(t, world):
    import torch.distributed as dist
    out = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(out, t.contiguous())
    return out


# --------------------------------------------------- 1 + 3: world 2, exact
W2_IDS = ([1, 2, 3, 12], [3, 4, 5, 12, 12])


def _dyadic_embedding(rows, dim, seed):
    torch.manual_seed(seed)
    emb = torch.nn.Embedding(rows, dim, sparse=True)
    with torch.no_grad():  # multiples of 2^-8: every sum below is exact
        emb.weight.copy_((emb.weight * 256).round() / 256)
    return emb


def _world2_run(rank, world, routing, steps=3):
    emb = _dyadic_embedding(20, 4, seed=7)
    opt = torch.optim.SGD(emb.parameters(), lr=0.5)
    # rows [0,10) owned by rank 0, rows [10,20) by rank 1
    _, engine = _engine(rank, world, emb, opt, owners=[0, 1], routing=routing)
    ids = torch.tensor(W2_IDS[rank])
    for _ in range(steps):
        opt.zero_grad()
        emb(ids).sum().backward()
        opt.step()
    engine.drain()
    stats = engine.stats()
    engine.teardown()
    return emb.weight.detach().clone(), stats


def _world2_parity_case(rank, world):
    w_routed, _ = _world2_run(rank, world, "owner")
    w_repl, _ = _world2_run(rank, world, "replicated")
    w0 = _dyadic_embedding(20, 4, seed=7).weight.detach()
    assert not torch.equal(w_routed[3], w0[3])      # it did train
    assert torch.equal(w_routed[0], w0[0])          # untouched row
    assert torch.equal(w_routed, w_repl), (w_routed - w_repl).abs().max()
    for other in _gather(w_routed, world):
        assert torch.equal(other, w_routed)         # replicas bit-identical


def test_world2_routed_equals_replicated_exactly():
    run_distributed(_world2_parity_case, world_size=2)


def _world2_stats_case(rank, world):
    """Rows received from OTHER ranks, from the definition:
    routed, rank 0 (owns rows 0-9): push = rank 1's coalesced ids {3,4,5}
    = 3, pull = rank 1's updated rows {12} = 1 -> 4; rank 1: push {12} = 1,
    pull {1,2,3,4,5} = 5 -> 6. Replicated: the other rank's raw nnz: rank 0
    receives 5, rank 1 receives 4."""
    _, st = _world2_run(rank, world, "owner", steps=2)
    assert st["sparse_routed_vars"] == 1
    assert st["sparse_vars"] == 1
    assert st["sparse_rows_received_last_step"] == (4, 6)[rank]
    _, st = _world2_run(rank, world, "replicated", steps=2)
    assert st["sparse_routed_vars"] == 0
    assert st["sparse_rows_received_last_step"] == (5, 4)[rank]


def test_world2_rows_received_stats():
    run_distributed(_world2_stats_case, world_size=2)


# ------------------------------------------- 2: world 4, uneven shards
def _w4_ids(step, rank):
    """Per-step ids with duplicates; step 1 touches no row of shard 2
    (rows 16-22) on any rank, so that shard's step counter must advance on
    an empty push."""
    gen = torch.Generator().manual_seed(100 * step + rank)
    ids = torch.randint(0, 30, (9,), generator=gen)
    if step == 1:
        ids = torch.where((ids >= 16) & (ids < 23), ids - 16, ids)
    return torch.cat([ids, ids[:2]])  # guaranteed duplicates


def _w4_run(rank, world, routing, opt_name, steps=4):
    torch.manual_seed(11)
    emb = torch.nn.Embedding(30, 5, sparse=True)
    if opt_name == "Adagrad":
        opt = torch.optim.Adagrad(emb.parameters(), lr=0.1, lr_decay=0.1)
    else:
        opt = torch.optim.Adam(emb.parameters(), lr=0.01)
    _, engine = _engine(rank, world, emb, opt, owners=[0, 1, 2, 3],
                        routing=routing)
    for step in range(steps):
        ids = _w4_ids(step, rank)
        gen = torch.Generator().manual_seed(7000 + 10 * step + rank)
        coef = torch.rand(ids.shape[0], 5, generator=gen) * 2 - 1
        opt.zero_grad()
        (emb(ids) * coef).sum().backward()
        opt.step()
    engine.drain()
    state = engine.consolidated_optimizer_state()
    return emb.weight.detach().clone(), state, engine


@pytest.mark.parametrize("opt_name", ["Adagrad", "Adam"])
def test_world4_uneven_shards_match_replicated(opt_name):
    run_distributed(_world4_case, world_size=4, args=(opt_name,))


def _world4_case(rank, world, opt_name):
    # the premise of the step-counter check: step 1 leaves shard 2 empty
    assert all(not ((_w4_ids(1, r) >= 16) & (_w4_ids(1, r) < 23)).any()
               for r in range(world))
    w_r, st_r, eng_r = _w4_run(rank, world, "owner", opt_name)
    w_p, st_p, eng_p = _w4_run(rank, world, "replicated", opt_name)
    assert eng_r.stats()["sparse_routed_vars"] == 1
    assert torch.allclose(w_r, w_p, atol=1e-6), (w_r - w_p).abs().max()
    (name,) = list(st_r)
    assert set(st_r[name]) == set(st_p[name]) and len(st_r[name]) >= 2
    for k, v in st_p[name].items():
        got = st_r[name][k]
        assert got.shape == v.shape, (k, got.shape, v.shape)
        assert torch.allclose(got.float().cpu(), v.float().cpu(),
                              atol=1e-6), k
    assert float(st_r[name]["step"]) == 4.0
    # shard-local state on owners only: lengths 8, 8, 7, 7
    (plan,) = eng_r.var_plans
    assert [sh.slice.length for sh in plan.shards] == [8, 8, 7, 7]
    for sh in plan.shards:
        if sh.owner_rank == rank:
            tensors = [t for t in sh.state.values() if t.dim() > 0]
            assert tensors
            assert all(t.shape == (sh.slice.length, 5) for t in tensors)
        else:
            assert sh.state is None
    for other in _gather(w_r, world):
        assert torch.equal(other, w_r)
    eng_r.teardown()
    eng_p.teardown()


# ------------------------------------------------------- 4: checkpoints
def _ckpt_batch(step, rank):
    gen = torch.Generator().manual_seed(300 + 10 * step + rank)
    ids = torch.randint(0, 20, (6,), generator=gen)
    coef = torch.rand(6, 4, generator=gen) * 2 - 1
    return ids, coef


def _ckpt_train(emb, opt, rank, steps, first=0):
    for step in range(first, first + steps):
        ids, coef = _ckpt_batch(step, rank)
        opt.zero_grad()
        (emb(ids) * coef).sum().backward()
        opt.step()


def _ckpt_setup(rank, world, routing, weight=None):
    torch.manual_seed(21)
    emb = torch.nn.Embedding(20, 4, sparse=True)
    if weight is not None:
        with torch.no_grad():
            emb.weight.copy_(weight)
    opt = torch.optim.Adagrad(emb.parameters(), lr=0.1, lr_decay=0.05)
    g, engine = _engine(rank, world, emb, opt, owners=[0, 1], routing=routing)
    return emb, opt, g, engine


def _checkpoint_case(rank, world, tmpdir):
    import torch.distributed as dist
    from autodist_amd.checkpoint.saver import Saver

    emb_r, opt_r, g_r, eng_r = _ckpt_setup(rank, world, "owner")
    saver = Saver(graph_item=g_r)
    emb_p, opt_p, _, eng_p = _ckpt_setup(rank, world, "replicated")
    _ckpt_train(emb_r, opt_r, rank, 2)
    _ckpt_train(emb_p, opt_p, rank, 2)
    full_r = eng_r.consolidated_optimizer_state()
    full_p = eng_p.consolidated_optimizer_state()
    (name,) = list(full_r)
    assert set(full_r[name]) == {"step", "sum"}
    assert full_r[name]["sum"].shape == (20, 4)
    assert float(full_r[name]["step"]) == 2.0
    assert torch.allclose(full_r[name]["sum"].cpu(), full_p[name]["sum"].cpu(),
                          atol=1e-6)
    # single-node compatible file
    path = saver.save(tmpdir + "/ckpt_routed")
    dist.barrier()
    w_saved = emb_r.weight.detach().clone()

    # fresh routed engine restored from the consolidated state: each owner
    # holds only its slice, and one more step matches the never-saved engine
    emb_2, opt_2, _, eng_2 = _ckpt_setup(rank, world, "owner", weight=w_saved)
    eng_2.load_optimizer_state(full_r)
    (plan,) = eng_2.var_plans
    for sh in plan.shards:
        if sh.owner_rank == rank:
            assert sh.state["sum"].shape == (10, 4)
            assert torch.equal(sh.state["sum"],
                               sh.slice.view(full_r[name]["sum"]))
        else:
            assert sh.state is None
    _ckpt_train(emb_r, opt_r, rank, 1, first=2)
    _ckpt_train(emb_2, opt_2, rank, 1, first=2)
    assert torch.equal(emb_2.weight, emb_r.weight)

    # the file loads into plain torch: continue with the global batch
    # (mean over ranks of the per-rank sums) and land on the same weights
    ckpt = torch.load(path, weights_only=False)
    vemb = torch.nn.Embedding(20, 4, sparse=True)
    vemb.load_state_dict(ckpt["model"])
    assert torch.equal(vemb.weight.detach(), w_saved)
    vopt = torch.optim.Adagrad(vemb.parameters(), lr=0.1, lr_decay=0.05)
    vopt.load_state_dict(ckpt["optimizer"])
    vopt.zero_grad()
    loss = 0
    for r in range(world):
        ids, coef = _ckpt_batch(2, r)
        loss = loss + (vemb(ids) * coef).sum() / world
    loss.backward()
    vopt.step()
    assert torch.allclose(vemb.weight.detach(), emb_r.weight.detach(),
                          atol=1e-6), \
        (vemb.weight.detach() - emb_r.weight.detach()).abs().max()
    for e in (eng_r, eng_p, eng_2):
        e.teardown()


def test_routed_checkpoint_roundtrip(tmp_path):
    run_distributed(_checkpoint_case, world_size=2, args=(str(tmp_path),))


# ------------------------------------------------- 5: eligibility and IR
def _stale_fallback_case(rank, world):
    emb = _dyadic_embedding(20, 4, seed=7)
    w0 = emb.weight.detach().clone()
    opt = torch.optim.SGD(emb.parameters(), lr=0.5)
    _, engine = _engine(rank, world, emb, opt, owners=[0, 1],
                        routing="owner", staleness=1)
    (plan,) = engine.var_plans
    assert not plan.routed
    assert engine.stats()["sparse_routed_vars"] == 0
    ids = torch.tensor(W2_IDS[rank])
    for _ in range(2):
        opt.zero_grad()
        emb(ids).sum().backward()
        opt.step()
    engine.drain()
    assert not torch.equal(emb.weight.detach()[3], w0[3])
    # the replicated path's result
    w_repl, _ = _world2_run(rank, world, "replicated", steps=2)
    assert torch.equal(emb.weight.detach(), w_repl)
    for other in _gather(emb.weight.detach(), world):
        assert torch.equal(other, emb.weight.detach())
    engine.teardown()


def test_stale_ps_falls_back_to_replicated():
    run_distributed(_stale_fallback_case, world_size=2)


def test_world1_without_collectives_is_not_routed():
    emb = _dyadic_embedding(20, 4, seed=7)
    opt = torch.optim.SGD(emb.parameters(), lr=0.5)
    _, engine = _engine(0, 1, emb, opt, owners=[0, 0], routing="owner")
    assert engine.stats()["sparse_routed_vars"] == 0
    opt.zero_grad()
    emb(torch.tensor([1, 1, 15])).sum().backward()
    opt.step()
    assert engine.stats()["sparse_rows_received_last_step"] == 0
    engine.teardown()


def test_ir_roundtrip_keeps_sparse_routing():
    from autodist_amd.proto.strategy_ir import (Node, PSSynchronizer,
                                                StrategyProto)
    proto = StrategyProto(id="x", node_config=[Node(
        var_name="emb", partitioner="2,1", part_config=[
            Node(var_name="emb/part_0", ps_synchronizer=PSSynchronizer(
                reduction_destination="a", sparse_routing="owner")),
            Node(var_name="emb/part_1", ps_synchronizer=PSSynchronizer(
                reduction_destination="b"))])])
    back = StrategyProto.parse_from_string(proto.serialize_to_string())
    parts = back.node_config[0].part_config
    assert parts[0].ps_synchronizer.sparse_routing == "owner"
    assert parts[1].ps_synchronizer.sparse_routing == "replicated"
    assert back.to_dict() == proto.to_dict()
    assert proto.to_dict()["node_config"][0]["part_config"][0][
        "ps_synchronizer"]["sparse_routing"] == "owner"


def test_ir_dict_without_key_loads_replicated_and_unknown_raises():
    from autodist_amd.proto.strategy_ir import PSSynchronizer
    old = {"reduction_destination": "a", "local_replication": False,
           "sync": True, "staleness": 0}
    assert PSSynchronizer.from_dict(old).sparse_routing == "replicated"
    with pytest.raises(ValueError):
        PSSynchronizer.from_dict({**old, "sparse_routing": "bogus"})
    with pytest.raises(ValueError):
        PSSynchronizer(sparse_routing="bogus")


BUILDERS = ["PS", "PSLoadBalancing", "PartitionedPS", "UnevenPartitionedPS",
            "Parallax"]


def _built_routings(builder):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.resource_spec import ResourceSpec
    emb = torch.nn.Embedding(20, 4, sparse=True)
    g = GraphItem()
    g.extend_model(emb)
    g.extend_optimizer_info(torch.optim.SGD(emb.parameters(), lr=0.5))
    strategy = builder.build(g, ResourceSpec())
    out = []
    for node in strategy.node_config:
        for n in (node.part_config or [node]):
            out.append(n.ps_synchronizer.sparse_routing)
    assert out
    return out


@pytest.mark.parametrize("builder_name", BUILDERS)
def test_builders_sparse_routing_keyword_and_env(builder_name, monkeypatch):
    from autodist_amd import strategy as strat
    cls = getattr(strat, builder_name)
    monkeypatch.delenv("AUTODIST_SPARSE_PS_ROUTING", raising=False)
    assert set(_built_routings(cls())) == {"replicated"}
    assert set(_built_routings(cls(sparse_routing="owner"))) == {"owner"}
    monkeypatch.setenv("AUTODIST_SPARSE_PS_ROUTING", "owner")
    assert set(_built_routings(cls())) == {"owner"}
    # an explicit keyword wins over the flag
    assert set(_built_routings(cls(sparse_routing="replicated"))) == {
        "replicated"}
    with pytest.raises(ValueError):
        cls(sparse_routing="bogus")
