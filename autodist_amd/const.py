"""Constants and environment flags.

MI355X-native re-derivation of the reference's constant/ENV surface
(reference: autodist/const.py:1-89). Same flag names where semantics carry
over, plus MI355X-specific tuning knobs (bucket bytes sized for xGMI links).
"""
import enum
import os

# Working directory for strategies / logs / traces (reference: const.py:20-27).
DEFAULT_WORKING_DIR = os.environ.get("AUTODIST_WORKING_DIR", "/tmp/autodist_amd")
DEFAULT_SERIALIZATION_DIR = os.path.join(DEFAULT_WORKING_DIR, "strategies")
DEFAULT_LOG_DIR = os.path.join(DEFAULT_WORKING_DIR, "logs")
DEFAULT_TRACE_DIR = os.path.join(DEFAULT_WORKING_DIR, "traces")
DEFAULT_GRAPH_DUMP_DIR = os.path.join(DEFAULT_WORKING_DIR, "graphs")

# Rendezvous port range (reference: const.py:38 uses 15000-16000 for TF servers).
DEFAULT_MASTER_PORT = 29517
DEFAULT_MASTER_ADDR = "127.0.0.1"

# Name prefixes kept for strategy/graph dump readability
# (reference: const.py:43-52 AutoDist-Replica etc. — we are process-per-GPU,
# so replica prefixes map to ranks).
AUTODIST_PREFIX = "AutoDist-"
REPLICA_PREFIX = "Rank-"

# MI355X tuning: xGMI is 7 point-to-point links x ~153 GB/s per GPU; ring
# collectives are per-link bound, so buckets must be large enough to amortize
# RCCL launch + protocol overhead but small enough to overlap with backward.
# 100 MiB measured as a good default for 8x ring on one node (re-tuned on HW).
DEFAULT_BUCKET_BYTES = 100 * 1024 * 1024
# First bucket smaller so the first collective launches early in backward.
DEFAULT_FIRST_BUCKET_BYTES = 8 * 1024 * 1024

MAX_INT32 = 2 ** 31 - 1


class ENV(enum.Enum):
    """Environment variable flags (reference: const.py:55-89, same protocol).

    Each member's value is a lambda returning the parsed value.
    """

    AUTODIST_WORKER = ((lambda v: v or ""),)                        # non-empty => this process is a worker, not chief
    AUTODIST_STRATEGY_ID = ((lambda v: v or ""),)                   # strategy id to load (worker side)
    AUTODIST_MIN_LOG_LEVEL = ((lambda v: v or "INFO"),)             # logger level
    AUTODIST_IS_TESTING = ((lambda v: v == "True" or v == "1"),)    # enable test-only checks
    AUTODIST_DEBUG_REMOTE = ((lambda v: v == "True" or v == "1"),)  # dry-run remote exec
    AUTODIST_RANK = ((lambda v: int(v) if v else None),)            # explicit rank override
    AUTODIST_RESOURCE_SPEC = ((lambda v: v or ""),)                 # path to resource spec yaml
    AUTODIST_SPARSE_PS_ROUTING = ((lambda v: v or "replicated"),)   # PS builders' default sparse_routing ("replicated" | "owner")
    AUTODIST_DENSE_AR_SCHEDULE = ((lambda v: v or "allreduce"),)    # AllReduce/Parallax builders' default schedule ("allreduce" | "sharded")

    @property
    def val(self):
        """Parsed value of the env var."""
        return self.value[0](os.environ.get(self.name))


def is_chief() -> bool:
    """A process is chief iff AUTODIST_WORKER is unset/empty and its rank is 0.

    Mirrors reference autodist.py:40-41; in process-per-GPU mode rank 0 of the
    launch is the chief.
    """
    if ENV.AUTODIST_WORKER.val:
        return False
    r = os.environ.get("RANK")
    if r is not None and int(r) != 0:
        return False
    return True
