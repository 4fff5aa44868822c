"""DistributedEngine — the per-rank execution engine.

This is the MI355X-native replacement for the reference's graph
transformation + TF distributed runtime. Where the reference rewrites a TF
GraphDef (GraphTransformer.transform, kernel/graph_transformer.py:55-92) and
lets TF's C++ executor run inserted CollectiveReduce / accumulator / queue
ops, this engine runs one process per GPU and installs the synchronization
directly:

  * AllReduce vars   -> flat gradient buckets + RCCL all-reduce on a comm
                        HIP stream, issued from post-accumulate-grad hooks so
                        collectives overlap backward
                        (reference: all_reduce_synchronizer.py:102-130); with
                        schedule="sharded": reduce-scatter, each rank updates
                        the 1/world bucket shard it owns with shard-local
                        optimizer state, then the parameters are all-gathered.
  * PS vars          -> shard owners hold a master copy + shard-local
                        optimizer state; reduce->apply->broadcast pipelined on
                        the comm stream with optional bounded staleness
                        (reference: ps_synchronizer.py:250-458).
  * Partitioned vars -> per-shard owners/buckets (partitioner.py semantics).
  * Sparse vars      -> variable-length allgather + segment-coalesce + rowwise
                        apply (reference: all_reduce_synchronizer.py:132-173,
                        ps_synchronizer.py:476-535); with
                        sparse_routing="owner" on a synchronous PS: rows are
                        pushed to their shard owner (all-to-all), applied
                        there with shard-local state, and the updated rows
                        pulled back (allgatherv).

The engine applies optimizer updates itself (parallel/apply.py) — required
for shard-local state — matching torch.optim numerics exactly.
"""
import dataclasses
import os
from typing import Dict, List, Optional

import torch
import torch.distributed as dist

from autodist_amd.const import DEFAULT_BUCKET_BYTES, DEFAULT_MASTER_ADDR, \
    DEFAULT_MASTER_PORT
from autodist_amd.parallel import apply as apply_mod
from autodist_amd.parallel.buckets import Bucket, build_buckets
from autodist_amd.parallel.comm import allgather_rows, alltoallv, \
    coalesce_rows
from autodist_amd.parallel.compressor import Compressor
from autodist_amd.parallel.partitioner import ShardSlice, \
    make_shard_slices, sorted_row_segments
from autodist_amd.proto.strategy_ir import CompressorType
from autodist_amd.utils import logging

@dataclasses.dataclass
class ShardPlan:
    name: str
    kind: str                      # "allreduce" | "ps"
    slice: Optional[ShardSlice]    # None = whole variable
    group: int = 0                 # AR bucket group
    owner_rank: int = 0            # PS owner
    compressor: CompressorType = CompressorType.NoneCompressor
    sync: bool = True
    staleness: int = 0
    local_replication: bool = False
    sparse_routing: str = "replicated"   # PS only: "replicated" | "owner"
    schedule: str = "allreduce"          # AR only: "allreduce" | "sharded"
    # runtime state
    state: Optional[dict] = None           # optimizer state (applier ranks)
    master: Optional[torch.Tensor] = None  # PS master copy (owner)
    stage: Optional[torch.Tensor] = None   # PS broadcast staging buffer
    reducer: Optional["ShardReducer"] = None


@dataclasses.dataclass
class VarPlan:
    name: str
    param: torch.nn.Parameter
    sparse: bool
    cls_name: str                  # optimizer class
    hyper: dict                    # LIVE optimizer hyperparams (shared per
                                   # param_group; refreshed every step so LR
                                   # schedulers take effect — see
                                   # engine._refresh_hyper)
    group_index: int = 0           # index into optimizer.param_groups
    shards: List[ShardPlan] = dataclasses.field(default_factory=list)
    bucketed: bool = False
    routed: bool = False           # sparse var on the owner-routed PS path
    shard_edges: Optional[torch.Tensor] = None  # routed: shard starts + end


class ShardReducer:
    """Direct all-reduce of one gradient shard (partitioned-AR path)."""

    def __init__(self, plan: ShardPlan, param: torch.nn.Parameter):
        self.plan = plan
        self.param = param
        self.compressor = Compressor.create(plan.compressor, plan.name)
        self._buf: Optional[torch.Tensor] = None
        self._handle = None
        self._issued = False
        self._is_view = False

    def reset(self):
        self._handle = None
        self._issued = False

    def _shard_grad(self):
        g = self.param.grad
        sl = self.plan.slice
        if sl is None:
            view = g
        else:
            view = sl.view(g)
        if view.is_contiguous():
            self._is_view = True
            return view
        self._is_view = False
        if self._buf is None or self._buf.shape != view.shape:
            self._buf = torch.empty_like(view, memory_format=torch.contiguous_format)
        self._buf.copy_(view)
        return self._buf

    def issue(self, engine):
        if self._issued:
            return
        # no gradient this step (unused param — consistently unused on every
        # rank since all ranks run the same graph): skip the collective
        if self.param.grad is None:
            return
        self._issued = True
        if not engine.collectives_active:
            return
        if engine.device.type == "cuda":
            ev = torch.cuda.Event()
            ev.record()
            engine.comm_stream.wait_event(ev)
            with torch.cuda.stream(engine.comm_stream):
                self._reduce(engine)
        else:
            self._reduce(engine)

    def _reduce(self, engine):
        t = self._shard_grad()
        self._handle = self.compressor.reduce(t, group=engine.process_group,
                                              async_op=True,
                                              scale=engine.grad_scale())
        self._reduced_tensor = t

    def finalize(self, engine):
        if not engine.collectives_active or not self._issued:
            return
        if engine.device.type == "cuda":
            with torch.cuda.stream(engine.comm_stream):
                self.compressor.finalize(self._reduced_tensor, self._handle)
                if not self._is_view:
                    self.plan.slice.view(self.param.grad).copy_(self._reduced_tensor)
            ev = torch.cuda.Event()
            ev.record(engine.comm_stream)
            torch.cuda.current_stream().wait_event(ev)
        else:
            self.compressor.finalize(self._reduced_tensor, self._handle)
            if not self._is_view:
                self.plan.slice.view(self.param.grad).copy_(self._reduced_tensor)


class DistributedEngine:
    """One rank's engine. Builds plans from a compiled Strategy and runs the
    per-step synchronization + update protocol."""

    def __init__(self, graph_item, strategy, rank: Optional[int] = None,
                 world_size: Optional[int] = None,
                 device: Optional[torch.device] = None,
                 bucket_bytes: int = DEFAULT_BUCKET_BYTES,
                 process_group=None):
        self.graph_item = graph_item
        self.strategy = strategy
        self.rank = rank if rank is not None else int(os.environ.get("RANK", 0))
        self.world_size = world_size if world_size is not None else int(
            os.environ.get("WORLD_SIZE", 1))
        self.process_group = process_group
        if device is not None:
            self.device = device
        elif torch.cuda.is_available():
            local = int(os.environ.get("LOCAL_RANK", self.rank % max(
                torch.cuda.device_count(), 1)))
            self.device = torch.device("cuda", local)
        else:
            self.device = torch.device("cpu")
        self.bucket_bytes = bucket_bytes
        self.comm_stream = None
        self.buckets: List[Bucket] = []
        self.var_plans: List[VarPlan] = []
        self._hook_handles = []
        self.ps_groups: list = []
        self._replica_ranks: Dict[str, int] = {}
        self._step_count = 0
        # logical rows this rank received from OTHER ranks in the last
        # step's sparse sync (padding excluded); see stats()
        self._sparse_rows_received = 0
        self._fallback_user_opt = False
        # sharded buckets run as "allreduce" because the user's own
        # optimizer.step() applies the update (see _build_buckets_and_hooks)
        self._sharded_downgraded = False
        self._setup_done = False
        self._accumulating = False
        # one SHARED live hyperparam dict per optimizer param_group; plans,
        # shards and buckets all alias these dicts so a per-step refresh
        # propagates LR-scheduler / manual param_groups changes everywhere
        self._group_hyper: Dict[int, dict] = {}
        # per-rank gradient weight for uneven batch splits: weighted average
        # sum_r (n_r / N) * g_r (reference c0.py:92-119). None => 1/world.
        self._batch_fraction: Optional[float] = None
        # AUTODIST_FORCE_COLLECTIVES=1: execute every RCCL collective even at
        # world_size==1 (sum over one rank == identity, so numerics are
        # unchanged). This is the 1-GPU hardware-validation mode: real
        # ncclAllReduce/Broadcast/Reduce/AllGather enqueue, comm-stream event
        # ordering, compressor wire handles and hipGraph x RCCL capture all
        # run exactly as they do at world 8 — RCCL itself refuses >1 rank
        # per device ("Duplicate GPU detected"), so this is the deepest
        # single-GPU proof available.
        self._force_collectives = os.environ.get(
            "AUTODIST_FORCE_COLLECTIVES", "") in ("1", "True")
        # AUTODIST_COMM_SAMPLES=<path>: record (nbytes, world, seconds)
        # comm-stream windows of every bucket all-reduce and dump JSON at
        # drain(). NOTE: these measure the full issue->finalize window
        # (includes queueing behind earlier buckets while overlapped with
        # backward) — an overlap/occupancy diagnostic. Bare-collective
        # calibration for the cost model comes from the serialized
        # tools/comm_microbench.py sweep instead.
        self._comm_sample_path = os.environ.get("AUTODIST_COMM_SAMPLES", "")
        self._comm_events: list = []
        # note: RCCL supports ReduceOp.AVG, but the mean is instead fused as
        # a scale into the compress/cast kernels (one code path for gloo +
        # every compressor)

    @property
    def comm_sampling(self) -> bool:
        return bool(self._comm_sample_path) and self.device.type == "cuda"

    def record_comm_sample(self, nbytes, ev0, ev1):
        self._comm_events.append((nbytes, ev0, ev1))

    def flush_comm_samples(self):
        """Resolve recorded events into (nbytes, world, seconds) samples and
        append them to AUTODIST_COMM_SAMPLES as JSON lines."""
        if not self._comm_events:
            return []
        torch.cuda.synchronize(self.device)
        samples = [(n, self.world_size, ev0.elapsed_time(ev1) / 1e3)
                   for n, ev0, ev1 in self._comm_events]
        self._comm_events.clear()
        if self._comm_sample_path:
            import json
            with open(self._comm_sample_path, "a") as f:
                for s_ in samples:
                    f.write(json.dumps(s_) + "\n")
        return samples

    @property
    def collectives_active(self) -> bool:
        """True when the engine issues real collectives (world>1, or the
        world-1 RCCL validation mode AUTODIST_FORCE_COLLECTIVES)."""
        return self.world_size > 1 or self._force_collectives

    # ------------------------------------------------------------------ set-up
    def maybe_init_process_group(self):
        if not self.collectives_active or dist.is_initialized():
            return
        backend = "nccl" if self.device.type == "cuda" else "gloo"
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
        addr = os.environ.get("MASTER_ADDR", DEFAULT_MASTER_ADDR)
        port = os.environ.get("MASTER_PORT", str(DEFAULT_MASTER_PORT))
        # generous timeout: the first collective can sit behind minutes of
        # MIOpen find-mode tuning on each rank
        import datetime
        dist.init_process_group(
            backend=backend, init_method=f"tcp://{addr}:{port}",
            rank=self.rank, world_size=self.world_size,
            timeout=datetime.timedelta(minutes=45))
        logging.info("process group ready: backend=%s rank=%d world=%d",
                     backend, self.rank, self.world_size)

    def setup(self):
        if self._setup_done:
            return self
        self.maybe_init_process_group()
        if self.device.type == "cuda":
            torch.cuda.set_device(self.device)
            self.comm_stream = torch.cuda.Stream(device=self.device)
        for m in self.graph_item.models:
            m.to(self.device)
        self._map_replica_ranks()
        self._build_plans()
        self._sync_initial_params()
        self._build_buckets_and_hooks()
        self._patch_optimizer()
        self.graph_item._engine = self  # checkpoint Saver discovery
        self._setup_done = True
        return self

    def _map_replica_ranks(self):
        for i, dev in enumerate(self.strategy.graph_config.replicas):
            self._replica_ranks[dev] = i

    def _owner_rank_of(self, destination: str) -> int:
        if destination in self._replica_ranks:
            return self._replica_ranks[destination]
        # CPU destination or unknown device: host rank 0 owns it
        return 0

    def _hyper_for(self, param) -> tuple:
        """(cls_name, live hyper dict, param_group index) for one param.

        The returned dict is SHARED by every param of the same group and is
        refreshed from the live optimizer each step (_refresh_hyper), so LR
        schedulers and manual param_groups edits keep torch.optim semantics."""
        opt_item = self.graph_item.optimizers[0] if self.graph_item.optimizers else None
        if opt_item is None:
            raise RuntimeError("no optimizer captured — build one inside scope()")
        opt = opt_item.optimizer
        if opt is not None:
            for gidx, group in enumerate(opt.param_groups):
                for p in group["params"]:
                    if p is param:
                        if gidx not in self._group_hyper:
                            self._group_hyper[gidx] = {
                                k: v for k, v in group.items()
                                if k != "params"}
                        return opt_item.cls_name, self._group_hyper[gidx], gidx
        if -1 not in self._group_hyper:
            self._group_hyper[-1] = dict(opt_item.defaults)
        return opt_item.cls_name, self._group_hyper[-1], -1

    def _refresh_hyper(self):
        """Re-read param_group hyperparams from the live optimizer (in place,
        so plan/shard/bucket aliases see the update). Fixes silent divergence
        under LR schedulers now that opt.step() routes through the engine."""
        opt_item = self.graph_item.optimizers[0] if self.graph_item.optimizers else None
        opt = opt_item.optimizer if opt_item else None
        if opt is None:
            return
        for gidx, group in enumerate(opt.param_groups):
            cur = self._group_hyper.get(gidx)
            if cur is None:
                continue
            for k, v in group.items():
                if k == "params":
                    continue
                if isinstance(v, torch.Tensor):  # capturable-style tensor lr
                    cur[k] = v
                elif cur.get(k) != v:
                    cur[k] = v

    def set_batch_fraction(self, fraction: Optional[float]):
        """Per-rank batch fraction n_r/N for the current step's gradients.
        Used as the gradient weight so uneven feed splits produce the exact
        weighted average (reference tests/integration/cases/c0.py:92-119)."""
        self._batch_fraction = fraction

    def grad_scale(self) -> float:
        """Weight applied to this rank's gradients before the summing
        collective: batch fraction if known, else 1/world."""
        if self._batch_fraction is not None:
            return float(self._batch_fraction)
        return 1.0 / self.world_size

    def _build_plans(self):
        vars_by_name = self.graph_item.trainable_var_op_to_var
        for node in self.strategy.node_config:
            item = vars_by_name.get(node.var_name)
            if item is None or item.param is None:
                continue
            cls_name, hyper, gidx = self._hyper_for(item.param)
            plan = VarPlan(name=node.var_name, param=item.param,
                           sparse=item.is_sparse, cls_name=cls_name,
                           hyper=hyper, group_index=gidx)
            if node.part_config and not getattr(
                    item.param, "_autodist_shard_local", False):
                slices = make_shard_slices(item.shape, node.partitioner)
                if len(slices) != len(node.part_config):
                    raise ValueError(
                        f"variable {node.var_name}: partitioner produced "
                        f"{len(slices)} shards but strategy has "
                        f"{len(node.part_config)} part_config entries")
                for sl, part in zip(slices, node.part_config):
                    plan.shards.append(self._make_shard(part, sl))
            else:
                plan.shards.append(self._make_shard(node, None,
                                                    param=item.param))
            if plan.sparse:
                plan.routed = self._sparse_routing_applies(plan)
            self.var_plans.append(plan)
        known = {p.name for p in self.var_plans}
        missing = [n for n in vars_by_name if n not in known
                   and vars_by_name[n].param is not None]
        if missing:
            logging.warning("vars without strategy config (treated as "
                            "local-only): %s", missing[:5])
        unsupported = {p.cls_name for p in self.var_plans
                       if not apply_mod.is_supported(p.cls_name)}
        if unsupported:
            all_simple_ar = all(
                len(p.shards) == 1 and p.shards[0].kind == "allreduce"
                and not p.sparse for p in self.var_plans)
            if not all_simple_ar:
                raise NotImplementedError(
                    f"optimizer(s) {unsupported} not supported by the engine "
                    "applier; PS/partitioned/sparse strategies need a torch "
                    "optimizer class with an engine apply (parallel/apply.py)")
            self._fallback_user_opt = True
            logging.info("unsupported optimizer %s: falling back to user "
                         "optimizer.step() after gradient sync", unsupported)

    def _make_shard(self, node, sl: Optional[ShardSlice],
                    param=None) -> ShardPlan:
        if param is not None and getattr(param, "_autodist_shard_local", False):
            # exclusively-owned shard (e.g. ShardedEmbedding): update locally,
            # never synchronize
            return ShardPlan(name=node.var_name, kind="local", slice=None)
        if node.all_reduce_synchronizer is not None:
            s = node.all_reduce_synchronizer
            return ShardPlan(name=node.var_name, kind="allreduce", slice=sl,
                             group=s.group, compressor=s.compressor,
                             schedule=s.schedule)
        if node.ps_synchronizer is not None:
            s = node.ps_synchronizer
            return ShardPlan(name=node.var_name, kind="ps", slice=sl,
                             owner_rank=self._owner_rank_of(s.reduction_destination),
                             sync=s.sync, staleness=s.staleness,
                             local_replication=s.local_replication,
                             sparse_routing=s.sparse_routing)
        # no synchronizer: local-only (treated as AR group 0 w/o collective)
        return ShardPlan(name=node.var_name, kind="allreduce", slice=sl)

    def _sparse_routing_applies(self, plan: VarPlan) -> bool:
        """Does this sparse variable take the owner-routed PS path? Only a
        fully synchronous PS placement with real collectives does; stale or
        async PS, allreduce-kind shards and world 1 without forced
        collectives keep the replicated path."""
        if not any(sh.kind == "ps" and sh.sparse_routing == "owner"
                   for sh in plan.shards):
            return False
        reason = None
        if not all(sh.kind == "ps" and sh.sparse_routing == "owner"
                   for sh in plan.shards):
            reason = "not every shard is an owner-routed PS shard"
        elif not all(sh.sync and sh.staleness == 0 for sh in plan.shards):
            reason = "stale/async PS"
        elif any(sh.slice is not None and sh.slice.axis != 0
                 for sh in plan.shards):
            reason = "shards are not split along the row axis"
        elif not self.collectives_active:
            reason = "no collectives at world size 1"
        if reason is not None:
            logging.info("sparse var %s: owner routing requested but not "
                         "applicable (%s); using the replicated path",
                         plan.name, reason)
            return False
        return True

    def _sync_initial_params(self):
        if not self.collectives_active:
            return
        for plan in self.var_plans:
            if getattr(plan.param, "_autodist_shard_local", False):
                continue  # exclusively-owned shard: shapes differ per rank
            dist.broadcast(plan.param.data, src=0, group=self.process_group)

    def _build_buckets_and_hooks(self):
        bucket_items = []
        ps_items = []
        hooked = set()
        for plan in self.var_plans:
            if plan.sparse:
                plan.param.grad = None
                continue
            whole = len(plan.shards) == 1 and plan.shards[0].slice is None
            sh0 = plan.shards[0]
            if sh0.kind == "local":
                sh0.state = apply_mod.make_state(plan.cls_name,
                                                 plan.param.data, plan.hyper)
                continue
            if whole and sh0.kind == "allreduce":
                plan.bucketed = True
                schedule = sh0.schedule
                if schedule == "sharded" and self._fallback_user_opt:
                    # the user's optimizer.step() needs the averaged gradient
                    # of every element on every rank
                    if not self._sharded_downgraded:
                        logging.warning(
                            "schedule='sharded' needs an optimizer class the "
                            "engine applies itself; %s is not one: running "
                            "those buckets with schedule='allreduce'",
                            plan.cls_name)
                    self._sharded_downgraded = True
                    schedule = sh0.schedule = "allreduce"
                # group_index in the key keeps buckets homogeneous in LIVE
                # param_group (two groups with equal initial hyper may
                # diverge later under a scheduler)
                bucket_items.append((plan.param, sh0.group, sh0.compressor,
                                     plan.cls_name, plan.hyper,
                                     (plan.group_index,
                                      _hyper_key(plan.hyper)), schedule))
            elif sh0.kind == "allreduce":
                # partitioned AR: per-shard direct reducers
                for sh in plan.shards:
                    sh.reducer = ShardReducer(sh, plan.param)
                if id(plan.param) not in hooked:
                    hooked.add(id(plan.param))
                    self._hook_handles.append(
                        plan.param.register_post_accumulate_grad_hook(
                            self._make_shard_hook(plan)))
            else:
                # PS shards: coalesced into per-owner flat groups below
                ps_items.extend((plan, sh) for sh in plan.shards)
                if id(plan.param) not in hooked:
                    hooked.add(id(plan.param))
                    self._hook_handles.append(
                        plan.param.register_post_accumulate_grad_hook(
                            self._make_ps_hook(plan)))
        # one reduce+broadcast per OWNER per step, hook-issued so PS traffic
        # overlaps backward (reference dataflow overlap,
        # ps_synchronizer.py:250-332; round-1 issued per-shard pairs)
        from autodist_amd.parallel.ps_synchronizer import PSSynchronizer
        self.ps_groups = PSSynchronizer.build_groups(self, ps_items)
        # PS/partitioned params keep ordinary grads; bucketed params get views
        self.buckets = build_buckets(bucket_items, self.device,
                                     self.bucket_bytes,
                                     world_size=self.world_size,
                                     rank=self.rank)
        # deterministic cross-rank collective keys (reference
        # collective_key.py:43-70): instance key = md5 of member var names,
        # group key = the replica device set; engine.step() flushes unissued
        # buckets in instance-key order so every rank enqueues RCCL
        # collectives identically regardless of hook timing
        from autodist_amd.parallel.collective_key import get_collective_keys
        ck = get_collective_keys()
        name_of = {id(pl.param): pl.name for pl in self.var_plans}
        devices = self.strategy.graph_config.replicas or [
            f"127.0.0.1:GPU:{r}" for r in range(self.world_size)]
        for b in self.buckets:
            members = ",".join(sorted(name_of.get(id(p), str(id(p)))
                                      for p in b.params))
            b.instance_key = ck.generate_instance_key(members)
            b.group_key = ck.generate_group_key(devices)
        param_to_bucket = {}
        for b in self.buckets:
            for p in b.params:
                param_to_bucket[id(p)] = b
        for plan in self.var_plans:
            if plan.bucketed:
                b = param_to_bucket[id(plan.param)]
                if id(plan.param) not in hooked:
                    hooked.add(id(plan.param))
                    self._hook_handles.append(
                        plan.param.register_post_accumulate_grad_hook(
                            self._make_bucket_hook(b)))
            elif plan.shards[0].kind == "allreduce" and plan.shards[0].reducer:
                for sh in plan.shards:
                    if sh.state is None:
                        ref = sh.slice.view(plan.param.data) if sh.slice \
                            else plan.param.data
                        sh.state = apply_mod.make_state(plan.cls_name, ref,
                                                        plan.hyper)

    def _make_bucket_hook(self, bucket: Bucket):
        def hook(_param):
            if self._accumulating:
                return
            bucket.mark_ready_and_maybe_issue(self)
        return hook

    def _make_shard_hook(self, plan: VarPlan):
        def hook(_param):
            if self._accumulating:
                return
            for sh in plan.shards:
                sh.reducer.issue(self)
        return hook

    def _make_ps_hook(self, plan: VarPlan):
        def hook(_param):
            if self._accumulating:
                return
            seen = set()  # a plan's shards may live in different owner groups
            for sh in plan.shards:
                grp = getattr(sh, "owner_group", None)
                if grp is not None and id(grp) not in seen:
                    seen.add(id(grp))
                    grp.mark_param_ready(self, plan)
        return hook

    def no_sync(self):
        """Context manager: skip gradient synchronization for accumulation
        micro-batches (grads accumulate into the flat buckets); the LAST
        backward runs outside it (DDP-style semantics)."""
        engine = self

        class _NoSync:
            def __enter__(self):
                engine._accumulating = True

            def __exit__(self, *exc):
                engine._accumulating = False
                return False

        return _NoSync()

    def _patch_optimizer(self):
        """Route the captured optimizer's step/zero_grad through the engine
        (the torch-idiom analog of the reference's apply_gradients patch,
        autodist/patch.py:79-88)."""
        opt = self.graph_item.optimizer
        if opt is None:
            return
        engine = self

        import types

        def step(_opt, closure=None):
            loss = None
            if closure is not None:
                # torch.optim contract: re-evaluate the model under grad
                # and return the loss (LBFGS-style loops)
                with torch.enable_grad():
                    loss = closure()
            engine.step()
            return loss

        def zero_grad(_opt, set_to_none=True):  # noqa: ARG001
            engine.zero_grad()

        # bound methods (not bare functions): torch LR schedulers wrap
        # opt.step and require __func__/__self__ on it
        opt._autodist_orig_step = opt.step
        opt.step = types.MethodType(step, opt)
        opt._autodist_orig_zero_grad = opt.zero_grad
        opt.zero_grad = types.MethodType(zero_grad, opt)

    # ------------------------------------------------------------------ steps
    def zero_grad(self):
        for b in self.buckets:
            b.zero_()
            b.reset()
        for plan in self.var_plans:
            if not plan.bucketed:
                plan.param.grad = None
                for sh in plan.shards:
                    if sh.reducer is not None:
                        sh.reducer.reset()

    def step(self):
        """Synchronize gradients + apply updates. Call after backward."""
        # 0) pick up live LR-scheduler / param_groups changes
        self._refresh_hyper()
        # 1) flush collectives not yet issued (e.g. params w/o grads) in
        #    instance-key order — deterministic across ranks regardless of
        #    hook timing (reference collective_key.py:60-70 semantics)
        for b in sorted(self.buckets, key=lambda b: b.instance_key):
            if not b._issued:
                b.issue(self)
        for plan in self.var_plans:
            for sh in plan.shards:
                if sh.reducer is not None:
                    sh.reducer.issue(self)
        # 2) finalize AR (compute stream now depends on reduced grads)
        for b in self.buckets:
            b.finalize(self)
        for plan in self.var_plans:
            for sh in plan.shards:
                if sh.reducer is not None:
                    sh.reducer.finalize(self)
        # 3) sparse path (var_plans order: the same collective sequence on
        #    every rank)
        self._sparse_rows_received = 0
        for plan in self.var_plans:
            if plan.routed:
                self._sync_and_apply_sparse_routed(plan)
            elif plan.sparse:
                self._sync_and_apply_sparse(plan)
        # 4) PS rounds: one reduce+apply+broadcast per owner group (those
        #    already hook-issued just complete; the rest flush here)
        for grp in self.ps_groups:
            grp.apply_and_broadcast(self)
        # 5) dense applies (AR vars) — grouped multi-tensor
        if self._fallback_user_opt:
            opt = self.graph_item.optimizer
            orig = getattr(opt, "_autodist_orig_step", opt.step)
            orig()
        else:
            self._apply_dense_updates()
        #    sharded buckets: the parameter all-gathers run on the comm
        #    stream; the next forward must see them
        if self.device.type == "cuda":
            for b in self.buckets:
                if b.gather_event is not None:
                    torch.cuda.current_stream().wait_event(b.gather_event)
        # 6) consume due PS rounds (staleness bound)
        for grp in self.ps_groups:
            grp.consume_due(self)
        # 7) reset per-step issue state HERE (not only in zero_grad): user
        #    code may call model.zero_grad(set_to_none=True) instead of the
        #    patched optimizer.zero_grad, which would leave _issued stuck
        for b in self.buckets:
            b.reset()
        for grp in self.ps_groups:
            grp.reset()
        for plan in self.var_plans:
            for sh in plan.shards:
                if sh.reducer is not None:
                    sh.reducer.reset()
        self._step_count += 1

    # -- dense AR apply ----------------------------------------------------
    def _apply_dense_updates(self):
        # bucketed params: one fused flat update per bucket. Instance-key
        # order: sharded buckets enqueue a collective each, and every rank
        # must enqueue the same sequence.
        for b in sorted(self.buckets, key=lambda b: b.instance_key):
            if not b.params:
                continue
            if b.sharded:
                # update only the shard this rank owns, straight from the
                # reduce-scattered (wire dtype) gradient shard; bucket i's
                # all-gather overlaps bucket i+1's update
                shard = b.param_shard()
                if not b.state:
                    b.state = apply_mod.make_state(b.cls_name, shard, b.hyper)
                apply_mod.apply_flat_shard(b.cls_name, shard,
                                           b.reduced_grad_shard(), b.state,
                                           b.hyper)
                if self.collectives_active:
                    b.gather_params(self)
                continue
            if not b.state:
                b.state = apply_mod.make_state(b.cls_name, b.flat_param, b.hyper)
            apply_mod.apply_flat(b.cls_name, b.flat_param, b.flat, b.state,
                                 b.hyper)
        # non-bucketed AR shards (partitioned): grouped multi-tensor
        groups: Dict[tuple, list] = {}
        for plan in self.var_plans:
            if plan.sparse or plan.bucketed:
                continue
            for sh in plan.shards:
                if sh.kind not in ("allreduce", "local"):
                    continue
                if plan.param.grad is None:  # unused param this step
                    continue
                if sh.slice is None:
                    p, g = plan.param.data, plan.param.grad
                else:
                    p = sh.slice.view(plan.param.data)
                    g = sh.slice.view(plan.param.grad)
                key = (plan.cls_name, _hyper_key(plan.hyper))
                groups.setdefault(key, []).append((p, g, sh.state, plan.hyper))
        for (cls_name, _), items in groups.items():
            params = [x[0] for x in items]
            grads = [x[1] for x in items]
            states = [x[2] for x in items]
            apply_mod.apply_dense(cls_name, params, grads, states, items[0][3])

    def drain(self):
        """Consume ALL outstanding PS rounds (end of training / checkpoint)."""
        for grp in self.ps_groups:
            grp.drain(self)
        if self.comm_sampling:
            self.flush_comm_samples()
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)

    # -- sparse path ---------------------------------------------------------
    @staticmethod
    def _sparse_grad_rows(grad):
        """(row ids, row values) of a sparse-flagged variable's gradient."""
        if grad.is_sparse:
            # use the RAW (possibly duplicated) rows: torch's coalesce() is
            # a full sort pass (rocprim radix/merge sorts were 37% of the
            # NCF step, measured), and rows dedup ONCE anyway in
            # coalesce_rows (segment-coalesce HIP kernel) after the gather
            indices, values = grad._indices()[0], grad._values()
        else:
            # dense grad on a sparse-flagged var: treat all rows as touched
            indices = torch.arange(grad.shape[0], device=grad.device)
            values = grad
        return indices, values

    def _sync_and_apply_sparse(self, plan: VarPlan):
        grad = plan.param.grad
        if grad is None:
            return
        indices, values = self._sparse_grad_rows(grad)
        # weight BEFORE the gather so uneven batch splits produce the exact
        # weighted average after cross-rank coalesce (c0.py:92-119 semantics)
        values = values * self.grad_scale()
        if self.collectives_active:
            idx_parts, val_parts, sizes = allgather_rows(
                indices, values, self.world_size, self.process_group,
                force=self._force_collectives)
            self._sparse_rows_received += sum(sizes) - sizes[self.rank]
            indices, values = torch.cat(idx_parts), torch.cat(val_parts)
        indices, values = coalesce_rows(indices, values)
        # replicated rowwise apply: identical on every rank == PS result
        sh = plan.shards[0]
        if sh.state is None:
            sh.state = apply_mod.make_state(plan.cls_name, plan.param.data,
                                            plan.hyper)
        cls = plan.cls_name
        if cls == "Adam" and plan.hyper.get("_sparse_adam"):
            cls = "SparseAdam"
        apply_mod.apply_sparse_rows(cls, plan.param.data, indices, values,
                                    sh.state, plan.hyper)

    def _sync_and_apply_sparse_routed(self, plan: VarPlan):
        """Owner-routed sparse PS round: push rows to their shard owners,
        apply there with shard-local state, pull the updated rows back.

        Wire volume per rank is its own coalesced rows out plus the owners'
        unique updated rows in, instead of every rank's raw rows; optimizer
        state exists only on shard owners. Replicas stay bit-identical: an
        owner's rows are what every other rank copies."""
        grad = plan.param.grad
        if grad is None:
            return
        world, group = self.world_size, self.process_group
        param = plan.param.data
        nrows = param.shape[0]
        indices, values = self._sparse_grad_rows(grad)
        # 1) weight (uneven batch splits), then dedup locally so each rank
        #    pushes a row at most once; coalesced ids come out sorted
        values = values * self.grad_scale()
        indices, values = coalesce_rows(indices, values)
        # 2) push: sorted ids make every shard one contiguous segment; a
        #    rank's part is the concatenation of the segments it owns
        if plan.shard_edges is None:
            edges = [sh.slice.start if sh.slice else 0 for sh in plan.shards]
            last = plan.shards[-1].slice
            edges.append(last.end if last else nrows)
            plan.shard_edges = torch.tensor(edges, dtype=torch.int64,
                                            device=indices.device)
        segments = sorted_row_segments(indices, plan.shard_edges)
        per_rank: List[list] = [[] for _ in range(world)]
        for sh, seg in zip(plan.shards, segments):
            per_rank[sh.owner_rank].append(seg)
        id_parts, val_parts = [], []
        for segs in per_rank:
            if len(segs) == 1:
                lo, hi = segs[0]
                id_parts.append(indices[lo:hi])
                val_parts.append(values[lo:hi])
            else:  # none (empty part) or several owned shards
                id_parts.append(torch.cat(
                    [indices[lo:hi] for lo, hi in segs] or [indices[:0]]))
                val_parts.append(torch.cat(
                    [values[lo:hi] for lo, hi in segs] or [values[:0]]))
        recv_ids, counts = alltoallv(id_parts, world, group)
        recv_vals, _ = alltoallv(val_parts, world, group,
                                 trailing_shape=tuple(values.shape[1:]),
                                 recv_sizes=counts)
        self._sparse_rows_received += sum(counts) - counts[self.rank]
        # 3) owner: sum what the ranks pushed, then one row-wise apply per
        #    owned shard. Every owned shard is applied EVERY step, rows or
        #    not: its step counter is the global step (Adagrad lr_decay, Adam
        #    bias correction), exactly as the replicated path advances it.
        own_ids, own_vals = coalesce_rows(torch.cat(recv_ids),
                                          torch.cat(recv_vals))
        own_vals = own_vals.contiguous()
        new_rows = torch.empty_like(own_vals)
        cls = plan.cls_name
        if cls == "Adam" and plan.hyper.get("_sparse_adam"):
            cls = "SparseAdam"
        for sh in plan.shards:
            if sh.owner_rank != self.rank:
                continue  # non-owners hold no state for this shard
            view = sh.slice.view(param) if sh.slice else param
            if sh.state is None:
                sh.state = apply_mod.make_state(plan.cls_name, view,
                                                plan.hyper)
            # ids of other owned shards fall outside [start, start+len) and
            # are skipped; each shard fills its own rows of new_rows
            apply_mod.apply_sparse_rows(
                cls, view, own_ids, own_vals, sh.state, plan.hyper,
                row_base=sh.slice.start if sh.slice else 0,
                new_rows=new_rows)
        # 4) pull: owners publish (global ids, updated rows); every other
        #    rank copies them into its replica bit for bit
        idx_parts, row_parts, sizes = allgather_rows(
            own_ids, new_rows, world, group, force=self._force_collectives)
        self._sparse_rows_received += sum(sizes) - sizes[self.rank]
        for r in range(world):
            if r != self.rank and sizes[r]:
                param.index_copy_(0, idx_parts[r], row_parts[r])

    # ----------------------------------------------------- checkpoint support
    def _state_keys(self, cls_name: str, hyper: dict):
        """Deterministic optimizer-state key list for one var/shard."""
        if cls_name == "SGD":
            return ["momentum_buffer"] if hyper.get("momentum", 0) else []
        if cls_name in ("Adam", "AdamW"):
            keys = ["step", "exp_avg", "exp_avg_sq"]
            if hyper.get("amsgrad"):
                keys.append("max_exp_avg_sq")
            return keys
        if cls_name == "Adagrad":
            return ["step", "sum"]
        if cls_name == "RMSprop":
            keys = ["square_avg"]
            if hyper.get("momentum", 0) > 0:
                keys.append("momentum_buffer")
            if hyper.get("centered"):
                keys.append("grad_avg")
            return keys
        if cls_name == "Adamax":
            return ["step", "exp_avg", "exp_inf"]
        if cls_name == "NAdam":
            return ["step", "mu_product", "exp_avg", "exp_avg_sq"]
        if cls_name == "RAdam":
            return ["step", "exp_avg", "exp_avg_sq"]
        if cls_name == "Adadelta":
            return ["step", "square_avg", "acc_delta"]
        if cls_name == "ASGD":
            return ["step", "eta", "mu", "ax"]
        if cls_name == "Rprop":
            return ["step", "prev", "step_size"]
        return []

    def consolidated_optimizer_state(self) -> Dict[str, dict]:
        """Full (unsharded) optimizer state per variable name, assembled on
        EVERY rank (PS shard states are broadcast from their owners).

        This is what makes checkpoints single-node compatible — the
        reference's SaveSliceInfo reassembly (partitioner.py:292-346).
        """
        out: Dict[str, dict] = {}
        gathered: Dict[tuple, torch.Tensor] = {}  # sharded-bucket state
        param_to_bucket = {}
        for b in self.buckets:
            for p, off in zip(b.params, b.offsets):
                param_to_bucket[id(p)] = (b, off)
        for plan in self.var_plans:
            keys = self._state_keys(plan.cls_name, plan.hyper)
            if not keys:
                out[plan.name] = {}
                continue
            state: dict = {}
            if plan.bucketed:
                b, off = param_to_bucket[id(plan.param)]
                n = plan.param.numel()
                for k in keys:
                    if k not in b.state:
                        continue
                    t = b.state[k]
                    if t.dim() == 0:  # shared step counter
                        state[k] = t.clone()
                        continue
                    if b.sharded and self.collectives_active:
                        # shard-local state: assemble the bucket's full
                        # tensor once, slice it per variable
                        if (b.id, k) not in gathered:
                            full = torch.empty(b.padded_numel, dtype=t.dtype,
                                               device=t.device)
                            dist.all_gather_into_tensor(
                                full, t.contiguous(),
                                group=self.process_group)
                            gathered[(b.id, k)] = full
                        t = gathered[(b.id, k)]
                    state[k] = t[off:off + n].view(plan.param.shape).clone()
            elif (plan.shards[0].kind == "local"
                  and getattr(plan.param, "_autodist_shard_range", None)
                  and self.world_size > 1):
                # exclusively-owned rows (ShardedEmbedding): assemble the full
                # per-row state across ranks (SaveSliceInfo semantics)
                from autodist_amd.parallel.comm import allgatherv
                sh = plan.shards[0]
                nrows = plan.param.shape[0]
                for k in keys:
                    t = (sh.state or {}).get(k)
                    if t is None:
                        continue
                    if t.dim() == 0 or t.shape[0] != nrows:
                        state[k] = t.clone()
                        continue
                    parts = allgatherv(t.detach().contiguous(),
                                       self.world_size, self.process_group)
                    state[k] = torch.cat(parts, dim=0).cpu()
            elif (plan.sparse and not plan.routed) or (
                    len(plan.shards) == 1
                    and plan.shards[0].kind in ("allreduce", "local")
                    and plan.shards[0].slice is None):
                sh = plan.shards[0]
                if sh.state:
                    for k in keys:
                        if k in sh.state:
                            state[k] = sh.state[k].clone()
            else:
                # sharded (partitioned AR or PS): assemble along the axis
                pieces: Dict[str, list] = {k: [] for k in keys}
                step_val = None
                for sh in plan.shards:
                    shard_shape = (sh.slice.view(plan.param.data).shape
                                   if sh.slice else plan.param.shape)
                    if sh.kind == "allreduce":
                        src_state = sh.state or {}
                        for k in keys:
                            if k == "step":
                                if k in src_state:
                                    step_val = src_state[k].clone()
                                continue
                            if k in src_state:
                                pieces[k].append(src_state[k])
                    else:  # PS shard: broadcast from owner
                        present = torch.zeros(len(keys), dtype=torch.uint8,
                                              device=self.device)
                        if self.rank == sh.owner_rank and sh.state:
                            for i, k in enumerate(keys):
                                present[i] = int(k in sh.state)
                        if self.world_size > 1:
                            dist.broadcast(present, src=sh.owner_rank,
                                           group=self.process_group)
                        for i, k in enumerate(keys):
                            if not bool(present[i]):
                                continue
                            if k == "step":
                                buf = torch.zeros((), device=self.device)
                                if self.rank == sh.owner_rank:
                                    buf.copy_(sh.state[k])
                                if self.world_size > 1:
                                    dist.broadcast(buf, src=sh.owner_rank,
                                                   group=self.process_group)
                                step_val = buf.cpu()
                                continue
                            buf = torch.zeros(shard_shape, device=self.device)
                            if self.rank == sh.owner_rank:
                                buf.copy_(sh.state[k])
                            if self.world_size > 1:
                                dist.broadcast(buf, src=sh.owner_rank,
                                               group=self.process_group)
                            pieces[k].append(buf)
                axis = plan.shards[0].slice.axis if plan.shards[0].slice else 0
                for k in keys:
                    if k == "step":
                        if step_val is not None:
                            state[k] = step_val
                    elif pieces[k]:
                        state[k] = torch.cat(
                            [t.to(self.device) for t in pieces[k]],
                            dim=axis).clone()
            out[plan.name] = state
        return out

    def load_optimizer_state(self, full_state: Dict[str, dict]):
        """Distribute a full optimizer-state dict back into bucket flats and
        shard owners (inverse of consolidated_optimizer_state)."""
        param_to_bucket = {}
        for b in self.buckets:
            for p, off in zip(b.params, b.offsets):
                param_to_bucket[id(p)] = (b, off)
        for plan in self.var_plans:
            state = full_state.get(plan.name) or {}
            if not state:
                continue
            keys = self._state_keys(plan.cls_name, plan.hyper)
            if plan.bucketed:
                b, off = param_to_bucket[id(plan.param)]
                n = plan.param.numel()
                lo, hi = b.shard_range
                if not b.state:
                    b.state = apply_mod.make_state(b.cls_name,
                                                   b.flat_param[lo:hi],
                                                   b.hyper)
                for k in keys:
                    if k not in state:
                        continue
                    src = state[k]
                    if k == "step":
                        b.state[k] = src.to(b.state.get(k, src).dtype) \
                            if "step" in b.state else src.clone()
                    elif b.sharded:
                        # write only what falls into this rank's shard
                        if k not in b.state:
                            b.state[k] = torch.zeros_like(b.flat[lo:hi])
                        a, z = max(off, lo), min(off + n, hi)
                        if a < z:
                            b.state[k][a - lo:z - lo].copy_(
                                src.reshape(-1)[a - off:z - off])
                    else:
                        if k not in b.state:
                            b.state[k] = torch.zeros_like(b.flat)
                        b.state[k][off:off + n].view(plan.param.shape).copy_(src)
            elif (plan.shards[0].kind == "local"
                  and getattr(plan.param, "_autodist_shard_range", None)):
                # slice the full per-row state back to the local rows
                rng = plan.param._autodist_shard_range
                sh = plan.shards[0]
                if sh.state is None:
                    sh.state = apply_mod.make_state(plan.cls_name,
                                                    plan.param.data, plan.hyper)
                for k in keys:
                    if k not in state:
                        continue
                    src = state[k]
                    if src.dim() == 0 or src.shape[0] != rng[2]:
                        sh.state[k] = src.clone().to(self.device)
                    else:
                        sh.state[k] = src[rng[0]:rng[1]].clone().to(self.device)
            else:
                axis = plan.shards[0].slice.axis if plan.shards[0].slice else 0
                for sh in plan.shards:
                    # replicated sparse vars apply on every rank; routed
                    # ones only on the shard owner, with the shard's slice
                    applies_here = (sh.kind == "allreduce"
                                    or self.rank == sh.owner_rank
                                    or (plan.sparse and not plan.routed))
                    if not applies_here:
                        continue
                    ref = sh.master if sh.master is not None else (
                        sh.slice.view(plan.param.data) if sh.slice
                        else plan.param.data)
                    if sh.state is None:
                        sh.state = apply_mod.make_state(plan.cls_name, ref,
                                                        plan.hyper)
                    for k in keys:
                        if k not in state:
                            continue
                        src = state[k]
                        if k == "step":
                            sh.state[k] = src.clone()
                        else:
                            piece = (sh.slice.view(src.to(self.device))
                                     if sh.slice else src.to(self.device))
                            sh.state[k] = piece.clone().contiguous()
                    if sh.master is not None:
                        view = sh.slice.view(plan.param.data) if sh.slice \
                            else plan.param.data
                        sh.master.copy_(view)
                        sh.stage.copy_(view)

    # ------------------------------------------------------------------ misc
    @property
    def step_count(self) -> int:
        return self._step_count

    def stats(self) -> dict:
        """Per-step synchronization accounting (observability — the
        reference had logging only, §5.5)."""
        ar_bytes = sum(b.nbytes for b in self.buckets if not b.sharded)
        sharded = [b for b in self.buckets if b.sharded]
        # per-element optimizer state this rank holds for bucketed variables
        # (1/world of it under the sharded schedule)
        state_bytes = sum(t.numel() * t.element_size()
                          for b in self.buckets for t in b.state.values()
                          if isinstance(t, torch.Tensor) and t.dim() > 0)
        ps_bytes = 0
        shard_reduce_bytes = 0
        n_ps_shards = 0
        n_reducers = 0
        for plan in self.var_plans:
            for sh in plan.shards:
                size = (sh.slice.view(plan.param.data).numel() if sh.slice
                        else plan.param.numel()) * plan.param.element_size()
                if sh.kind == "ps":
                    ps_bytes += size
                    n_ps_shards += 1
                elif sh.reducer is not None:
                    shard_reduce_bytes += size
                    n_reducers += 1
        return {
            "step_count": self._step_count,
            "world_size": self.world_size,
            "n_buckets": len(self.buckets),
            "allreduce_bytes_per_step": ar_bytes,
            "sharded_buckets": len(sharded),
            "sharded_downgraded": self._sharded_downgraded,
            "reduce_scatter_bytes_per_step": sum(
                b.reduce_scatter_nbytes for b in sharded),
            "allgather_bytes_per_step": sum(
                b.allgather_nbytes for b in sharded),
            "dense_optimizer_state_bytes_local": state_bytes,
            "ps_shards": n_ps_shards,
            "ps_owner_groups": len(self.ps_groups),
            "ps_collectives_per_step": 2 * len(self.ps_groups),
            "ps_bytes_per_step": ps_bytes,
            "partitioned_ar_shards": n_reducers,
            "partitioned_ar_bytes_per_step": shard_reduce_bytes,
            "sparse_vars": sum(1 for p in self.var_plans if p.sparse),
            "sparse_routed_vars": sum(1 for p in self.var_plans if p.routed),
            "sparse_rows_received_last_step": self._sparse_rows_received,
            "fallback_user_optimizer": self._fallback_user_opt,
        }

    def teardown(self):
        for h in self._hook_handles:
            h.remove()
        self._hook_handles.clear()
        opt = self.graph_item.optimizer
        if opt is not None and hasattr(opt, "_autodist_orig_step"):
            opt.step = opt._autodist_orig_step
        if opt is not None and hasattr(opt, "_autodist_orig_zero_grad"):
            opt.zero_grad = opt._autodist_orig_zero_grad


def _hyper_key(hyper: dict) -> tuple:
    out = []
    for k in sorted(hyper):
        v = hyper[k]
        if isinstance(v, (list, tuple)):
            v = tuple(v)
        elif not isinstance(v, (int, float, bool, str, type(None))):
            v = str(v)
        out.append((k, v))
    return tuple(out)
