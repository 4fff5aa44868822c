"""Multi-process (gloo) tests of the sharded dense schedule.

Two engines are built from identically seeded models in the same processes,
one with schedule="allreduce" and one with schedule="sharded", and fed the
same data. The model has 66 parameters (Linear(5,7) -> Tanh -> Linear(7,3)),
not a multiple of 8*world, so the pad and the shard cuts through variables
are live. Each case runs twice: one bucket (defaults), and four small buckets
(bucket_bytes=64 with one variable per strategy group; a single group would
stay one bucket, because the first bucket of an engine has a cap of its own).

Where a sum has two terms, or all terms but one are exact zeros, its value
does not depend on the order a backend adds in, and the two schedules must
agree bit for bit.
"""
import pytest
import torch

from tests.dist_utils import run_distributed

pytestmark = pytest.mark.integration

LAYOUTS = [({}, {}), ({"bucket_bytes": 64}, {"chunk_size": 1})]

OPTIMIZERS = {
    "sgdm": lambda ps: torch.optim.SGD(ps, lr=0.1, momentum=0.9,
                                       weight_decay=1e-2),
    "adamw": lambda ps: torch.optim.AdamW(ps, lr=1e-2),
    "adagrad": lambda ps: torch.optim.Adagrad(ps, lr=0.1),
    "rmsprop": lambda ps: torch.optim.RMSprop(ps, lr=1e-2),
    "sgd_lr1": lambda ps: torch.optim.SGD(ps, lr=1.0),
}


def _model():
    torch.manual_seed(11)  # same init on all ranks and for both engines
    return torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Tanh(),
                               torch.nn.Linear(7, 3))


def _engine(rank, world, schedule, opt_name, compressor, engine_kw,
            builder_kw, opt_factory=None):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.resource_spec import ResourceSpec
    from autodist_amd.strategy import AllReduce
    model = _model()
    g = GraphItem()
    g.extend_model(model)
    opt = (opt_factory or OPTIMIZERS[opt_name])(model.parameters())
    g.extend_optimizer_info(opt)
    strategy = AllReduce(compressor=compressor, schedule=schedule,
                         **builder_kw).build(g, ResourceSpec())
    strategy.graph_config.replicas = [
        f"127.0.0.1:CPU:{r}" for r in range(world)]
    engine = DistributedEngine(g, strategy, rank=rank, world_size=world,
                               device=torch.device("cpu"), **engine_kw)
    engine.setup()
    return model, opt, engine


def _pair(rank, world, opt_name, compressor, layout, opt_factory=None):
    engine_kw, builder_kw = layout
    return [_engine(rank, world, sched, opt_name, compressor, engine_kw,
                    builder_kw, opt_factory)
            for sched in ("allreduce", "sharded")]


def _train_step(model, opt, x, y, weight=1.0):
    opt.zero_grad()
    (torch.nn.functional.mse_loss(model(x), y) * weight).backward()
    opt.step()


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _assert_params_bitwise(model_a, model_b, what):
    for (name, pa), pb in zip(model_a.named_parameters(),
                              model_b.parameters()):
        assert torch.equal(_bits(pa), _bits(pb)), \
            f"{what}: {name} differs by {(pa - pb).abs().max().item()}"


def _assert_equal_across_ranks(model, world):
    import torch.distributed as dist
    for name, p in model.named_parameters():
        parts = [torch.empty_like(p) for _ in range(world)]
        dist.all_gather(parts, p.detach().contiguous())
        for q in parts:
            assert torch.equal(_bits(q), _bits(p)), \
                f"{name} differs across ranks"


def _feed(rank, step):
    torch.manual_seed(1000 + 17 * step + rank)  # per-rank, per-step data
    return torch.randn(8, 5), torch.randn(8, 3)


# ---------------------------------------------------- world 2: bitwise parity
def _world2_case(rank, world, opt_name, compressor):
    for layout in LAYOUTS:
        (m_ar, o_ar, e_ar), (m_sh, o_sh, e_sh) = _pair(
            rank, world, opt_name, compressor, layout)
        for step in range(3):
            x, y = _feed(rank, step)
            _train_step(m_ar, o_ar, x, y)
            _train_step(m_sh, o_sh, x, y)
            _assert_params_bitwise(m_ar, m_sh, f"{layout} step {step}")
        _assert_equal_across_ranks(m_sh, world)
        _check_layout_and_stats(e_ar, e_sh, world, compressor, layout)
        e_ar.teardown()
        e_sh.teardown()


def _check_layout_and_stats(e_ar, e_sh, world, compressor, layout):
    from autodist_amd.parallel.buckets import sharded_layout
    assert len(e_sh.buckets) == (4 if layout[0] else 1)
    wire_elt = 4 if compressor == "NoneCompressor" else 2
    padded_total, state_bytes = 0, 0
    for b in e_sh.buckets:
        padded, shard_len = sharded_layout(b.numel, world)
        assert b.sharded and b.padded_numel == padded
        assert b.flat.numel() == padded and b.flat_param.numel() == padded
        padded_total += padded
        per_element = [t for t in b.state.values() if t.dim() > 0]
        assert per_element, "every optimizer here keeps per-element state"
        for t in per_element:  # state exists for the owned shard alone
            assert t.numel() == shard_len
            state_bytes += 4 * shard_len
        # the pad belongs to no parameter and stays zero
        assert not b.flat_param[b.numel:].any()
    st = e_sh.stats()
    assert st["sharded_buckets"] == len(e_sh.buckets)
    assert st["reduce_scatter_bytes_per_step"] == padded_total * wire_elt
    assert st["allgather_bytes_per_step"] == padded_total * 4
    assert st["allreduce_bytes_per_step"] == 0
    assert st["dense_optimizer_state_bytes_local"] == state_bytes
    assert st["sharded_downgraded"] is False
    st = e_ar.stats()
    assert st["sharded_buckets"] == 0
    assert st["reduce_scatter_bytes_per_step"] == 0
    assert st["allgather_bytes_per_step"] == 0
    assert st["allreduce_bytes_per_step"] == 66 * 4
    n_state = len([t for t in e_ar.buckets[0].state.values() if t.dim() > 0])
    assert st["dense_optimizer_state_bytes_local"] == n_state * 66 * 4


@pytest.mark.parametrize("compressor", ["NoneCompressor", "HorovodCompressor",
                                        "HorovodCompressorEF"])
@pytest.mark.parametrize("opt_name", ["sgdm", "adamw", "adagrad", "rmsprop"])
def test_world2_bitwise_parity(opt_name, compressor):
    run_distributed(_world2_case, world_size=2, args=(opt_name, compressor))


# ------------------------------ world 3 and 4: sums that are exact in any order
def _one_contributor_case(rank, world, opt_name):
    for layout in LAYOUTS:
        (m_ar, o_ar, _e1), (m_sh, o_sh, _e2) = _pair(
            rank, world, opt_name, "NoneCompressor", layout)
        for step in range(2 * world):
            # only one rank contributes; the others' gradients are exact
            # zeros, so the sum is exact whatever order the backend adds in
            weight = 1.0 if rank == step % world else 0.0
            x, y = _feed(rank, step)
            _train_step(m_ar, o_ar, x, y, weight)
            _train_step(m_sh, o_sh, x, y, weight)
            _assert_params_bitwise(m_ar, m_sh, f"{layout} step {step}")
        _assert_equal_across_ranks(m_sh, world)


@pytest.mark.parametrize("opt_name", ["adamw", "sgdm"])
@pytest.mark.parametrize("world", [3, 4])
def test_world3_4_bitwise_parity_exact_sums(world, opt_name):
    run_distributed(_one_contributor_case, world_size=world,
                    args=(opt_name,))


# ------------------------------------------- world 4: general random feeds
def _world4_random_case(rank, world):
    import torch.distributed as dist
    for layout in LAYOUTS:
        engine_kw, builder_kw = layout
        model, opt, engine = _engine(rank, world, "sharded", "sgd_lr1",
                                     "NoneCompressor", engine_kw, builder_kw)
        p0 = [p.detach().clone() for p in model.parameters()]
        x, y = _feed(rank, 0)
        _train_step(model, opt, x, y)
        for p, before in zip(model.parameters(), p0):
            # sharded schedule: .grad is this rank's SCALED LOCAL gradient
            g = p.grad.detach().contiguous()
            parts = [torch.empty_like(g) for _ in range(world)]
            dist.all_gather(parts, g)
            exact = sum(q.double() for q in parts)
            mag = sum(q.double().abs() for q in parts)
            moved = before.double() - p.detach().double()
            # first-order bound of a world-term fp32 sum in any order, plus
            # the rounding of the final subtract (lr = 1)
            bound = (world - 1) * 2.0 ** -23 * mag \
                + 2.0 ** -24 * before.double().abs()
            err = (moved - exact).abs()
            print("world4 random: max err", err.max().item(),
                  "min slack", (bound - err).min().item())
            assert bool((err <= bound).all()), (err - bound).max().item()
            assert bool((mag > 0).any())
        _assert_equal_across_ranks(model, world)


def test_world4_random_feeds_within_fp32_sum_bound():
    run_distributed(_world4_random_case, world_size=4)


# ------------------------- uneven batch fractions, no_sync, fallback optimizer
class _UserSGD(torch.optim.SGD):
    """An optimizer class the engine cannot apply itself."""


def _misc_world2_case(rank, world):
    # uneven batch fractions: weighted average, bitwise as all-reduce
    for layout in LAYOUTS:
        (m_ar, o_ar, e_ar), (m_sh, o_sh, e_sh) = _pair(
            rank, world, "adamw", "NoneCompressor", layout)
        for e in (e_ar, e_sh):
            e.set_batch_fraction(0.25 if rank == 0 else 0.75)
        for step in range(2):
            x, y = _feed(rank, step)
            n = 2 if rank == 0 else 6
            _train_step(m_ar, o_ar, x[:n], y[:n])
            _train_step(m_sh, o_sh, x[:n], y[:n])
        _assert_params_bitwise(m_ar, m_sh, f"batch fraction {layout}")
        _assert_equal_across_ranks(m_sh, world)
    # no_sync(): two micro-batches accumulate, then one synchronized step
    for layout in LAYOUTS:
        pair = _pair(rank, world, "sgdm", "NoneCompressor", layout)
        for _ in range(2):
            for model, opt, engine in pair:
                opt.zero_grad()
                x, y = _feed(rank, 5)
                with engine.no_sync():
                    torch.nn.functional.mse_loss(model(x), y).backward()
                x, y = _feed(rank, 6)
                torch.nn.functional.mse_loss(model(x), y).backward()
                opt.step()
        _assert_params_bitwise(pair[0][0], pair[1][0], f"no_sync {layout}")
        _assert_equal_across_ranks(pair[1][0], world)
    # an optimizer class without an engine apply: downgraded, still correct
    (m_ar, o_ar, e_ar), (m_sh, o_sh, e_sh) = _pair(
        rank, world, None, "NoneCompressor", LAYOUTS[0],
        opt_factory=lambda ps: _UserSGD(ps, lr=0.1, momentum=0.9))
    assert e_sh._fallback_user_opt
    st = e_sh.stats()
    assert st["sharded_downgraded"] is True and st["sharded_buckets"] == 0
    assert st["allreduce_bytes_per_step"] == 66 * 4
    assert e_ar.stats()["sharded_downgraded"] is False
    for step in range(2):
        x, y = _feed(rank, step)
        _train_step(m_ar, o_ar, x, y)
        _train_step(m_sh, o_sh, x, y)
    _assert_params_bitwise(m_ar, m_sh, "fallback optimizer")


def test_world2_batch_fraction_no_sync_and_fallback():
    run_distributed(_misc_world2_case, world_size=2)


# ------------------------------------------------------------- checkpoints
def _checkpoint_case(rank, world):
    for layout in LAYOUTS:
        (m_ar, o_ar, e_ar), (m_sh, o_sh, e_sh) = _pair(
            rank, world, "adamw", "NoneCompressor", layout)
        for step in range(2):
            x, y = _feed(rank, step)
            _train_step(m_ar, o_ar, x, y)
            _train_step(m_sh, o_sh, x, y)
        ck_ar = e_ar.consolidated_optimizer_state()
        ck_sh = e_sh.consolidated_optimizer_state()
        # identical in structure and bits: interchangeable checkpoints
        assert list(ck_ar) == list(ck_sh) and len(ck_ar) == 4
        for name in ck_ar:
            assert list(ck_ar[name]) == list(ck_sh[name]), name
            assert list(ck_ar[name]) == ["step", "exp_avg", "exp_avg_sq"]
            for k, t in ck_ar[name].items():
                u = ck_sh[name][k]
                assert t.shape == u.shape and t.dtype == u.dtype, (name, k)
                assert torch.equal(_bits(t), _bits(u)), (name, k)
        # load each checkpoint into a fresh engine of the OTHER schedule
        (m_ar2, o_ar2, e_ar2), (m_sh2, o_sh2, e_sh2) = _pair(
            rank, world, "adamw", "NoneCompressor", layout)
        with torch.no_grad():
            for fresh, trained in ((m_ar2, m_sh), (m_sh2, m_ar)):
                for p, q in zip(fresh.parameters(), trained.parameters()):
                    p.copy_(q)
        e_ar2.load_optimizer_state(ck_sh)
        e_sh2.load_optimizer_state(ck_ar)
        for b in e_sh2.buckets:  # only the owned shard was written
            assert b.state["exp_avg"].numel() == b.shard_len
        x, y = _feed(rank, 9)
        for model, opt in ((m_ar, o_ar), (m_sh, o_sh), (m_ar2, o_ar2),
                           (m_sh2, o_sh2)):
            _train_step(model, opt, x, y)
        for other, what in ((m_sh, "sharded"), (m_ar2, "allreduce<-sharded"),
                            (m_sh2, "sharded<-allreduce")):
            _assert_params_bitwise(m_ar, other, f"{what} {layout}")
        _assert_equal_across_ranks(m_sh2, world)


def test_world2_checkpoints_interchangeable_between_schedules():
    run_distributed(_checkpoint_case, world_size=2)
