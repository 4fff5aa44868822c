"""PS with load balancing: greedy bin-pack variables onto servers by bytes.

Reference behavior: autodist/strategy/ps_lb_strategy.py:42-117
(byte_size_load_fn greedy packing). MI355X re-derivation: the candidate PS
set is every GPU (one rank per GPU) — sharding parameter ownership across all
8 GPUs spreads both the reduction traffic over all xGMI links and the
optimizer-state memory (ZeRO-style), instead of packing onto per-node CPUs.
"""
from autodist_amd.proto.strategy_ir import Node, PSSynchronizer
from autodist_amd.strategy.base import (Strategy, StrategyBuilder,
                                        resolve_sparse_routing)


def byte_size_load_fn(var_item) -> float:
    """Load function: variable size in bytes (reference ps_lb_strategy.py:88-117)."""
    return float(max(var_item.bytesize, 1))


class PSLoadBalancing(StrategyBuilder):
    """Greedy least-loaded assignment of vars to PS devices
    (reference ps_lb_strategy.py:42-86)."""

    def __init__(self, local_proxy_variable=False, sync=True, staleness=0,
                 sparse_routing=None):
        self._local_proxy_variable = local_proxy_variable
        self._sync = sync
        self._staleness = staleness
        self._sparse_routing = resolve_sparse_routing(sparse_routing)
        if staleness > 0:
            assert sync, "staleness is only valid for sync training"
        self.loads = {}

    def build(self, graph_item, resource_spec) -> Strategy:
        strategy = Strategy()
        gpus = [k for k, _ in resource_spec.gpu_devices]
        strategy.graph_config.replicas = gpus or [
            k for k, _ in resource_spec.cpu_devices[:1]]
        ps_devices = gpus or [resource_spec.node_cpu_device(n).name_string()
                              for n in resource_spec.nodes]
        self.loads = {d: 0.0 for d in ps_devices}
        strategy.node_config = [
            self._gen_ps_node_config(v)
            for v in graph_item.trainable_var_op_to_var.values()]
        return strategy

    def _gen_ps_node_config(self, var_item) -> Node:
        device = min(self.loads, key=self.loads.get)
        self.loads[device] += byte_size_load_fn(var_item)
        return Node(var_name=var_item.name, ps_synchronizer=PSSynchronizer(
            reduction_destination=device,
            local_replication=self._local_proxy_variable,
            sync=self._sync, staleness=self._staleness,
            sparse_routing=self._sparse_routing))
