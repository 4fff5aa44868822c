"""Gradient compressors for the all-reduce path.

Reference behavior: autodist/kernel/synchronization/compressor.py:84-284
(strategy pattern around the collective: NoneCompressor pass-through,
HorovodCompressor fp-cast, HorovodCompressorEF error feedback, PowerSGD
low-rank stub).

MI355X-native design: compressors operate on the BUCKET's flat tensor (not
per-variable) so one cast kernel + one RCCL call covers the whole group.
The cast runs on the comm stream so it overlaps backward compute; on GPU the
cast/EF kernels are hand-written HIP (ops.compress) and PowerSGD's two GEMMs
are MFMA-tiled (ops.powersgd) with rocBLAS fallback.
"""
from typing import Optional

import torch
import torch.distributed as dist

from autodist_amd.proto.strategy_ir import CompressorType


class Compressor:
    """Base: compress -> all_reduce -> decompress on a flat bucket tensor
    (reference Compressor.create pattern, compressor.py:98-112)."""

    def __init__(self, var_name: str = ""):
        self.var_name = var_name

    @classmethod
    def create(cls, kind: CompressorType, var_name: str = "",
               **kwargs) -> "Compressor":
        if kind == CompressorType.NoneCompressor:
            return NoneCompressor(var_name)
        if kind == CompressorType.HorovodCompressor:
            return HorovodCompressor(var_name)
        if kind == CompressorType.HorovodCompressorEF:
            return HorovodCompressorEF(var_name)
        if kind == CompressorType.PowerSGDCompressor:
            from autodist_amd.parallel.powersgd import PowerSGDCompressor
            return PowerSGDCompressor(var_name, **kwargs)
        raise ValueError(f"unknown compressor {kind}")

    def reduce(self, flat: torch.Tensor, group=None, async_op: bool = False,
               scale: float = 1.0):
        """All-reduce the flat gradient tensor; `scale` (typically 1/world)
        is FUSED into the compress kernel so the mean costs no extra pass
        (reference _all_reduce, compressor.py:84-96). Returns an async handle."""
        raise NotImplementedError

    def finalize(self, flat: torch.Tensor, handle) -> None:
        """Complete an async reduce (decompress back into `flat`)."""
        if handle is not None:
            handle.wait()

    # -- sharded schedule: reduce-scatter instead of all-reduce ------------
    def reduce_scatter(self, flat: torch.Tensor, world: int, group=None,
                       async_op: bool = False, scale: float = 1.0):
        """Same front half as `reduce` (scale / compress over the whole
        flat), then reduce-scatter: rank r receives the sum of elements
        [r*L, (r+1)*L), L = numel/world, in a persistent shard buffer kept
        in the WIRE dtype (nothing is cast back). Returns a handle for
        `finalize_shard`."""
        raise NotImplementedError(
            f"{type(self).__name__} has no reduce-scatter form")

    def finalize_shard(self, handle) -> torch.Tensor:
        """Complete an async reduce_scatter; returns the reduced shard."""
        h, shard = handle
        if h is not None:
            h.wait()
        return shard

    def _shard_buf(self, src: torch.Tensor, world: int) -> torch.Tensor:
        n = src.numel() // world
        buf = getattr(self, "_shard", None)
        if buf is None or buf.numel() != n or buf.dtype != src.dtype \
                or buf.device != src.device:
            buf = self._shard = torch.empty(n, dtype=src.dtype,
                                            device=src.device)
        return buf

    def _scatter(self, src, world, group, async_op):
        shard = self._shard_buf(src, world)
        handle = dist.reduce_scatter_tensor(shard, src, op=dist.ReduceOp.SUM,
                                            group=group, async_op=async_op)
        return (handle, shard)

    @property
    def wire_dtype(self) -> Optional[torch.dtype]:
        """Element type on the wire; None = the bucket's own dtype."""
        return None


class NoneCompressor(Compressor):
    """Pass-through all-reduce (reference compressor.py:146-166)."""

    def reduce_scatter(self, flat, world, group=None, async_op=False,
                       scale=1.0):
        if scale != 1.0:
            flat.mul_(scale)
        return self._scatter(flat, world, group, async_op)

    def reduce(self, flat, group=None, async_op=False, scale=1.0):
        if scale != 1.0:
            flat.mul_(scale)
        handle = dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group,
                                 async_op=async_op)
        return handle


class HorovodCompressor(Compressor):
    """Cast-compress to bf16 on the wire (reference compressor.py:169-201;
    the reference casts fp32->fp16, we use bf16: same 2x wire saving, no
    range loss, native CDNA4 dtype). The scale+cast is one fused gfx950
    kernel (ops/csrc/multi_tensor.hip scale_cast_bf16_kernel)."""

    WIRE_DTYPE = torch.bfloat16

    def __init__(self, var_name: str = ""):
        super().__init__(var_name)
        self._wire: Optional[torch.Tensor] = None

    def _wire_buf(self, flat: torch.Tensor) -> torch.Tensor:
        if self._wire is None or self._wire.numel() != flat.numel() \
                or self._wire.device != flat.device:
            self._wire = torch.empty_like(flat, dtype=self.WIRE_DTYPE)
        return self._wire

    def reduce(self, flat, group=None, async_op=False, scale=1.0):
        from autodist_amd.ops import api as ops_api
        wire = self._wire_buf(flat)
        ops_api.scale_cast_bf16(flat, wire, scale)
        handle = dist.all_reduce(wire, op=dist.ReduceOp.SUM, group=group,
                                 async_op=async_op)
        return (handle, wire)

    def finalize(self, flat, handle) -> None:
        from autodist_amd.ops import api as ops_api
        h, wire = handle
        if h is not None:
            h.wait()
        ops_api.cast_back_f32(wire, flat)

    @property
    def wire_dtype(self):
        return self.WIRE_DTYPE

    def reduce_scatter(self, flat, world, group=None, async_op=False,
                       scale=1.0):
        from autodist_amd.ops import api as ops_api
        wire = self._wire_buf(flat)
        ops_api.scale_cast_bf16(flat, wire, scale)
        return self._scatter(wire, world, group, async_op)


class HorovodCompressorEF(HorovodCompressor):
    """Cast compression with error feedback (reference compressor.py:204-205):
    error = flat - decompress(compress(flat)) is added back next step.
    accumulate+cast+error-update run as ONE fused kernel on gfx950."""

    def __init__(self, var_name: str = ""):
        super().__init__(var_name)
        self._error: Optional[torch.Tensor] = None

    def reduce(self, flat, group=None, async_op=False, scale=1.0):
        from autodist_amd.ops import api as ops_api
        if self._error is None:
            self._error = torch.zeros_like(flat)
        wire = self._wire_buf(flat)
        ops_api.ef_compress(flat, self._error, wire, scale)
        handle = dist.all_reduce(wire, op=dist.ReduceOp.SUM, group=group,
                                 async_op=async_op)
        return (handle, wire)

    def reduce_scatter(self, flat, world, group=None, async_op=False,
                       scale=1.0):
        from autodist_amd.ops import api as ops_api
        if self._error is None:
            self._error = torch.zeros_like(flat)
        wire = self._wire_buf(flat)
        ops_api.ef_compress(flat, self._error, wire, scale)
        return self._scatter(wire, world, group, async_op)
