"""CPU units of the sharded dense schedule (reduce-scatter, shard-local
update, all-gather): the strategy-IR field, the builder keyword and its
environment default, the padded bucket layout, and the shard apply's
dispatch by gradient dtype."""
import copy

import pytest
import torch

from autodist_amd.proto.strategy_ir import (AllReduceSynchronizer,
                                            CompressorType, Node,
                                            StrategyProto)


# ------------------------------------------------------------------ IR
def test_ir_roundtrip_keeps_schedule():
    proto = StrategyProto(id="s", node_config=[
        Node(var_name="a", all_reduce_synchronizer=AllReduceSynchronizer(
            group=1, schedule="sharded")),
        Node(var_name="b", all_reduce_synchronizer=AllReduceSynchronizer())])
    assert proto.to_dict()["node_config"][0]["all_reduce_synchronizer"][
        "schedule"] == "sharded"
    back = StrategyProto.parse_from_string(proto.serialize_to_string())
    assert back.node_config[0].all_reduce_synchronizer.schedule == "sharded"
    assert back.node_config[1].all_reduce_synchronizer.schedule == "allreduce"
    assert back.to_dict() == proto.to_dict()


def test_ir_missing_key_loads_as_allreduce_and_unknown_raises():
    old = {"spec": 1, "compressor": 0, "group": 3}
    sync = AllReduceSynchronizer.from_dict(old)
    assert sync.schedule == "allreduce" and sync.group == 3
    assert AllReduceSynchronizer().schedule == "allreduce"
    with pytest.raises(ValueError):
        AllReduceSynchronizer.from_dict({**old, "schedule": "bogus"})
    with pytest.raises(ValueError):
        AllReduceSynchronizer(schedule="bogus")


def test_ir_sharded_rejects_powersgd_only():
    with pytest.raises(ValueError):
        AllReduceSynchronizer(compressor=CompressorType.PowerSGDCompressor,
                              schedule="sharded")
    for comp in (CompressorType.NoneCompressor,
                 CompressorType.HorovodCompressor,
                 CompressorType.HorovodCompressorEF):
        assert AllReduceSynchronizer(
            compressor=comp, schedule="sharded").schedule == "sharded"
    # PowerSGD stays valid on the all-reduce schedule
    AllReduceSynchronizer(compressor=CompressorType.PowerSGDCompressor)


# ------------------------------------------------------------- builders
def _built_schedules(builder):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.resource_spec import ResourceSpec
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Embedding(16, 4, sparse=True),
                                torch.nn.Linear(4, 2))
    g = GraphItem()
    g.extend_model(model)
    g.extend_optimizer_info(torch.optim.SGD(model.parameters(), lr=0.1))
    strategy = builder.build(g, ResourceSpec())
    return [n.all_reduce_synchronizer.schedule for n in strategy.node_config
            if n.all_reduce_synchronizer is not None]


@pytest.mark.parametrize("builder_name", ["AllReduce", "Parallax"])
def test_builders_schedule_keyword_and_env(builder_name, monkeypatch):
    from autodist_amd import strategy as strat
    cls = getattr(strat, builder_name)
    monkeypatch.delenv("AUTODIST_DENSE_AR_SCHEDULE", raising=False)
    got = _built_schedules(cls())
    assert got and set(got) == {"allreduce"}
    assert set(_built_schedules(cls(schedule="sharded"))) == {"sharded"}
    monkeypatch.setenv("AUTODIST_DENSE_AR_SCHEDULE", "sharded")
    assert set(_built_schedules(cls())) == {"sharded"}
    # an explicit keyword wins over the environment
    assert set(_built_schedules(cls(schedule="allreduce"))) == {"allreduce"}
    with pytest.raises(ValueError):
        cls(schedule="bogus")
    monkeypatch.setenv("AUTODIST_DENSE_AR_SCHEDULE", "bogus")
    with pytest.raises(ValueError):
        cls()


@pytest.mark.parametrize("builder_name", ["AllReduce", "Parallax"])
def test_builders_reject_sharded_powersgd_at_build_time(builder_name,
                                                        monkeypatch):
    from autodist_amd import strategy as strat
    cls = getattr(strat, builder_name)
    monkeypatch.delenv("AUTODIST_DENSE_AR_SCHEDULE", raising=False)
    with pytest.raises(ValueError):
        cls(schedule="sharded", compressor="PowerSGDCompressor")
    cls(compressor="PowerSGDCompressor")  # default schedule: still fine
    for comp in ("NoneCompressor", "HorovodCompressor",
                 "HorovodCompressorEF"):
        assert cls(schedule="sharded", compressor=comp).schedule == "sharded"


def test_partitioned_builders_do_not_take_the_keyword():
    from autodist_amd import strategy as strat
    for name in ("PartitionedAR", "RandomAxisPartitionAR"):
        with pytest.raises(TypeError):
            getattr(strat, name)(schedule="sharded")


def test_env_flag_default(monkeypatch):
    from autodist_amd.const import ENV
    monkeypatch.delenv("AUTODIST_DENSE_AR_SCHEDULE", raising=False)
    assert ENV.AUTODIST_DENSE_AR_SCHEDULE.val == "allreduce"
    monkeypatch.setenv("AUTODIST_DENSE_AR_SCHEDULE", "sharded")
    assert ENV.AUTODIST_DENSE_AR_SCHEDULE.val == "sharded"


# --------------------------------------------------------------- layout
@pytest.mark.parametrize("world", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("numel", [1, 66, 1024])
def test_padding_and_ownership_arithmetic(numel, world):
    from autodist_amd.parallel.buckets import shard_bounds, sharded_layout
    padded, shard_len = sharded_layout(numel, world)
    assert padded >= numel and padded % (8 * world) == 0
    assert padded - numel < 8 * world          # no more pad than needed
    assert shard_len * world == padded
    edges = [shard_bounds(numel, world, r) for r in range(world)]
    assert edges[0][0] == 0 and edges[-1][1] == padded
    for (lo, hi), (nlo, _) in zip(edges, edges[1:]):
        assert hi == nlo                       # shards tile the buffer
    for lo, hi in edges:
        assert hi - lo == shard_len and lo % 8 == 0


@pytest.mark.parametrize("world,rank", [(1, 0), (3, 1), (4, 3)])
def test_bucket_allocates_the_padded_layout(world, rank):
    from autodist_amd.parallel.buckets import build_buckets, sharded_layout
    from autodist_amd.proto.strategy_ir import CompressorType as CT
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(),
                                torch.nn.Linear(7, 3))
    want = [p.detach().clone() for p in model.parameters()]
    items = [(p, 0, CT.NoneCompressor, "SGD", {}, (), "sharded")
             for p in model.parameters()]
    (b,) = build_buckets(items, torch.device("cpu"), world_size=world,
                         rank=rank)
    padded, shard_len = sharded_layout(66, world)
    assert b.sharded and b.numel == 66 and b.padded_numel == padded
    assert b.flat.numel() == padded and b.flat_param.numel() == padded
    assert b.shard_range == (rank * shard_len, (rank + 1) * shard_len)
    assert b.param_shard().numel() == shard_len
    assert b.param_shard().data_ptr() == b.flat_param.data_ptr() \
        + 4 * rank * shard_len
    # the pad is zero and belongs to no parameter; values are preserved
    assert not b.flat[66:].any() and not b.flat_param[66:].any()
    assert sum(p.numel() for p in b.params) == 66
    for p, w in zip(model.parameters(), want):
        assert torch.equal(p.detach(), w)
    # an item without the field is an all-reduce bucket, unpadded
    lin = torch.nn.Linear(5, 7)
    (b2,) = build_buckets([(p, 0, CT.NoneCompressor, "SGD", {}, ())
                           for p in lin.parameters()], torch.device("cpu"),
                          world_size=world, rank=rank)
    assert not b2.sharded and b2.flat.numel() == 42
    assert b2.shard_range == (0, 42)


def test_schedule_joins_the_bucket_key():
    from autodist_amd.parallel.buckets import build_buckets
    from autodist_amd.proto.strategy_ir import CompressorType as CT
    lin = torch.nn.Linear(5, 7)
    w, bias = lin.parameters()
    buckets = build_buckets(
        [(w, 0, CT.NoneCompressor, "SGD", {}, (), "sharded"),
         (bias, 0, CT.NoneCompressor, "SGD", {}, (), "allreduce")],
        torch.device("cpu"), world_size=2, rank=0)
    assert sorted(b.schedule for b in buckets) == ["allreduce", "sharded"]


# ---------------------------------------------------------- shard apply
_APPLY_CASES = [
    ("SGD", {"lr": 0.1, "momentum": 0.9, "weight_decay": 1e-2}),
    ("AdamW", {"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8,
               "weight_decay": 1e-2}),
    ("Adagrad", {"lr": 0.1, "lr_decay": 1e-2, "eps": 1e-10}),
]


@pytest.mark.parametrize("cls_name,hyper", _APPLY_CASES)
def test_apply_flat_shard_cpu_bf16_equals_apply_dense(cls_name, hyper):
    from autodist_amd.parallel import apply as apply_mod
    torch.manual_seed(1)
    n = 40
    p_a = torch.randn(n)
    p_b = p_a.clone()
    st_a = apply_mod.make_state(cls_name, p_a, hyper)
    st_b = copy.deepcopy(st_a)
    for _ in range(3):
        g = torch.randn(n).to(torch.bfloat16)
        apply_mod.apply_flat_shard(cls_name, p_a, g, st_a, hyper)
        apply_mod.apply_dense(cls_name, [p_b], [g.float()], [st_b], hyper)
    assert torch.equal(p_a, p_b)
    assert st_a.keys() == st_b.keys()
    for k in st_a:
        assert torch.equal(st_a[k], st_b[k]), k
    # an fp32 gradient takes the ordinary flat path
    g = torch.randn(n)
    apply_mod.apply_flat_shard(cls_name, p_a, g, st_a, hyper)
    apply_mod.apply_flat(cls_name, p_b, g, st_b, hyper)
    assert torch.equal(p_a, p_b)
