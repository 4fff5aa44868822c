"""Variable partitioner: axis-split of a variable + its gradient + optimizer
state across devices.

Reference behavior: autodist/kernel/partitioner.py:153-704 (delete var +
optimizer subgraph, re-create PartitionedVariable shards, split dense grads
by tf.slice / sparse by index-mod, fix savers via SaveSliceInfo).

MI355X-native design: every rank keeps the FULL parameter replica for compute
(data-parallel forward stays untouched, like the reference's identity-concat
read, partitioner.py:577-602), but gradient synchronization and optimizer
state are SHARDED: each shard has its own owner/bucket, and only the applier
rank materializes that shard's optimizer state (ZeRO-style memory saving on
288 GB HBM3E). Shard boundaries follow torch.tensor_split semantics: the
first (dim0 % n) shards get one extra row — which also covers the
reference's "uneven partition" strategy.

Sparse shards route rows by range: shard i owns rows [start_i, end_i), and
sparse gradient rows are rebased by -start_i (the reference's floor_mod
rebasing, partitioner.py:661-684, re-derived for range sharding).
"""
import dataclasses
from typing import List, Tuple

import torch


@dataclasses.dataclass
class ShardSlice:
    """One shard's slab: [start, end) along `axis` of the full variable."""
    axis: int
    start: int
    end: int

    @property
    def length(self) -> int:
        return self.end - self.start

    def view(self, tensor: torch.Tensor) -> torch.Tensor:
        """A view of the shard inside the full tensor (contiguous iff axis 0)."""
        return tensor.narrow(self.axis, self.start, self.length)


def split_boundaries(dim: int, n: int) -> List[Tuple[int, int]]:
    """torch.tensor_split boundaries: first (dim % n) shards get +1."""
    n = max(1, min(n, dim))
    base, extra = divmod(dim, n)
    out = []
    start = 0
    for i in range(n):
        ln = base + (1 if i < extra else 0)
        out.append((start, start + ln))
        start += ln
    return out


def make_shard_slices(shape, partitioner: str) -> List[ShardSlice]:
    """Parse a strategy partitioner string ("n,1,..") into shard slices."""
    counts = [int(x) for x in partitioner.split(",") if x]
    axis = 0
    n = 1
    for ax, c in enumerate(counts):
        if c > 1:
            axis, n = ax, c
            break
    if n <= 1 or not shape:
        return [ShardSlice(0, 0, shape[0] if shape else 1)]
    return [ShardSlice(axis, s, e) for s, e in split_boundaries(shape[axis], n)]


def sorted_row_segments(sorted_ids: torch.Tensor, edges: torch.Tensor
                        ) -> List[Tuple[int, int]]:
    """Per-shard [lo, hi) positions inside SORTED global row ids.

    `edges` holds the shards' first rows followed by the last shard's end
    (len = n_shards + 1, ascending, same device as the ids). Sorted ids make
    every shard one contiguous segment, so routing is a binary search per
    edge and one host read instead of route_sparse_rows' mask per shard; ids
    outside [edges[0], edges[-1]) fall in no segment.
    """
    cuts = torch.searchsorted(sorted_ids, edges).tolist()
    return list(zip(cuts[:-1], cuts[1:]))


def route_sparse_rows(indices: torch.Tensor, values: torch.Tensor,
                      slices: List[ShardSlice]):
    """Route sparse gradient rows to shards with index rebasing
    (reference _split_indexed_slices_v2, partitioner.py:661-684).

    Returns [(local_indices, local_values)] per shard; local indices are
    rebased to shard-local coordinates.
    """
    out = []
    for sl in slices:
        mask = (indices >= sl.start) & (indices < sl.end)
        rows = indices[mask] - sl.start
        out.append((rows, values[mask]))
    return out
