"""Collective helpers: variable-length allgather and friends.

Reference context: sparse gradients synchronize via two collective_ops
all_gather calls on indices/values (all_reduce_synchronizer.py:132-173).
RCCL has no allgatherv; this implements size-exchange + padded allgather,
with the padding trimmed on unpack (the standard xGMI-friendly schedule:
one small int64 allgather + one large padded allgather). The variable-length
all-to-all (alltoallv) serves ShardedEmbedding's id/vector exchange and the
owner-routed sparse PS push.
"""
from typing import List, Tuple

import torch
import torch.distributed as dist


def allgatherv(tensor: torch.Tensor, world_size: int, group=None,
               force: bool = False) -> List[torch.Tensor]:
    """All-gather tensors whose dim-0 length differs per rank.

    Returns the per-rank tensors (views of one padded buffer, trimmed).
    `force` executes the real collectives even at world_size==1 (the 1-GPU
    RCCL validation mode, AUTODIST_FORCE_COLLECTIVES).
    """
    if world_size <= 1 and not force:
        return [tensor]
    return _allgather_padded(tensor, _exchange_sizes(tensor, world_size, group),
                             world_size, group)


def _exchange_sizes(tensor: torch.Tensor, world_size: int, group=None
                    ) -> List[int]:
    """Every rank's dim-0 length of `tensor`, as host ints."""
    n_local = torch.tensor([tensor.shape[0]], dtype=torch.int64,
                           device=tensor.device)
    sizes = torch.zeros(world_size, dtype=torch.int64, device=tensor.device)
    dist.all_gather_into_tensor(sizes, n_local, group=group)
    return sizes.tolist()


def _allgather_padded(tensor: torch.Tensor, sizes_l: List[int],
                      world_size: int, group=None) -> List[torch.Tensor]:
    """Padded allgather of `tensor` given every rank's dim-0 length."""
    max_n = max(sizes_l) if sizes_l else 0
    if max_n == 0:
        return [tensor[:0] for _ in range(world_size)]
    pad_shape = (max_n,) + tuple(tensor.shape[1:])
    padded = torch.zeros(pad_shape, dtype=tensor.dtype, device=tensor.device)
    padded[:tensor.shape[0]] = tensor
    flat_in = padded.reshape(-1)
    out = torch.zeros(world_size * flat_in.numel(), dtype=tensor.dtype,
                      device=tensor.device)
    dist.all_gather_into_tensor(out, flat_in, group=group)
    out = out.view((world_size,) + pad_shape)
    return [out[r, :sizes_l[r]] for r in range(world_size)]


def allgather_sparse(indices: torch.Tensor, values: torch.Tensor,
                     world_size: int, group=None, force: bool = False
                     ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Gather a row-sparse gradient (indices [nnz], values [nnz, dim...])
    from all ranks; returns concatenated (indices, values)."""
    idx_parts, val_parts, _ = allgather_rows(indices, values, world_size,
                                             group, force=force)
    return torch.cat(idx_parts), torch.cat(val_parts)


def allgather_rows(indices: torch.Tensor, values: torch.Tensor,
                   world_size: int, group=None, force: bool = False
                   ) -> Tuple[List[torch.Tensor], List[torch.Tensor],
                              List[int]]:
    """allgatherv of (indices [n], values [n, dim...]) pairs with ONE size
    exchange for both. Returns (per-rank indices, per-rank values, per-rank
    row counts); the counts are host ints, so callers can account traffic
    without another synchronisation."""
    if world_size <= 1 and not force:
        return [indices], [values], [int(indices.shape[0])]
    sizes_l = _exchange_sizes(indices, world_size, group)
    return (_allgather_padded(indices, sizes_l, world_size, group),
            _allgather_padded(values, sizes_l, world_size, group), sizes_l)


def alltoallv(parts, world, group, trailing_shape=(), recv_sizes=None):
    """Exchange variable-length dim-0 chunks; parts[r] goes to rank r.
    Returns (received chunks as a list per source rank, their lengths).
    `recv_sizes` (the lengths returned by an earlier call whose parts had the
    same dim-0 lengths, e.g. the ids that go with these values) skips the
    size exchange."""
    dev = parts[0].device
    send_list = [int(p.shape[0]) for p in parts]
    if recv_sizes is None:
        send_sizes = torch.tensor(send_list, dtype=torch.int64).to(dev)
        recv_sizes_t = torch.zeros_like(send_sizes)
        dist.all_to_all_single(recv_sizes_t, send_sizes, group=group)
        recv_list = recv_sizes_t.tolist()
    else:
        recv_list = list(recv_sizes)
    total_recv = sum(recv_list)
    flat_send = torch.cat(parts, dim=0)
    out = torch.empty((total_recv,) + tuple(trailing_shape),
                      dtype=flat_send.dtype, device=dev)
    dist.all_to_all_single(out, flat_send, recv_list, send_list, group=group)
    offs = [0]
    for n in recv_list:
        offs.append(offs[-1] + n)
    return [out[offs[r]:offs[r + 1]] for r in range(world)], recv_list


def coalesce_rows(indices: torch.Tensor, values: torch.Tensor
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Sum duplicate rows (the reference's sparse-accumulator dedup,
    ps_synchronizer.py:498-535). On gfx950 the segmented-reduce HIP kernel
    (ops/csrc/sparse_ops.hip) replaces the sort+index_add composite."""
    if indices.numel() == 0:
        return indices, values
    from autodist_amd.ops import api as ops_api
    if ops_api.has_gpu_ops() and indices.is_cuda:
        return ops_api.segment_coalesce(indices, values)
    uniq, inv = torch.unique(indices, sorted=True, return_inverse=True)
    out = torch.zeros((uniq.shape[0],) + tuple(values.shape[1:]),
                      dtype=values.dtype, device=values.device)
    out.index_add_(0, inv, values)
    return uniq, out
