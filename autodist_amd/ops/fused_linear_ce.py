"""Linear layer + cross-entropy with an ignore index in one op: the BERT
masked-LM head loss.

    z[n]    = h[n] W^T + b                  only for rows with a label
    loss[n] = logsumexp(z[n]) - z[n, t_n]   0 where labels[n] == ignore_index

On the GPU with bf16 compute `fused_linear_cross_entropy` runs the lce_* HIP
kernels (ops/csrc/lce_ops.hip): the labelled rows are compacted on the
device (a scan, no host read of their number), the logits of those rows are
formed tile by tile on bf16 MFMA with the online log-sum-exp as the epilogue
and are never stored, and backward recomputes them into dz [M_cap, V] bf16
and the bias gradient.

What stays on hipBLASLt through torch, as in sampled_softmax.py: dHc = dz W
and dW = dz^T Hc (one GEMM each), and an index_copy that puts dHc back into
the rows of dh.

Everything else (CPU, fp32 compute, a shape the kernels refuse, a step under
stream capture) runs the torch composite F.linear + F.cross_entropy.
`AUTODIST_LINEAR_CE=torch` forces the composite.
"""
import os

import torch
import torch.nn.functional as F

from autodist_amd.ops import api as ops_api

_MAX_K = 1024


def _bf16_compute(h):
    return h.is_cuda and (
        h.dtype == torch.bfloat16
        or (torch.is_autocast_enabled()
            and torch.get_autocast_dtype("cuda") == torch.bfloat16))


def _aligned16(t):
    return t.data_ptr() % 16 == 0


def can_use_lce_kernels(h, weight, bias):
    """True when the HIP kernels serve this call: a contiguous, 16-byte
    aligned h [..., K] on the GPU with bf16 compute (a bf16 h, or bf16
    autocast on), K a multiple of 32 up to 1024, an fp32 or bf16 weight
    [V, K] with V >= 2 and a bias [V] or None on the same GPU (a bf16 weight
    is read in place, so it must be contiguous and aligned), the extension
    loaded, no stream capture in progress (the composed BERT graph faults on
    replay with custom backward kernels in it, see fused_linear) and
    AUTODIST_LINEAR_CE not "torch"."""
    if os.environ.get("AUTODIST_LINEAR_CE") == "torch":
        return False
    if not (_bf16_compute(h) and ops_api.has_gpu_ops()):
        return False
    if torch.cuda.is_current_stream_capturing():
        return False
    K = h.size(-1)
    return (h.numel() >= K and h.is_contiguous() and _aligned16(h)
            and K % 32 == 0 and 32 <= K <= _MAX_K
            and h.dtype in (torch.float32, torch.bfloat16)
            and weight.dim() == 2 and weight.device == h.device
            and weight.size(1) == K and weight.size(0) >= 2
            and (weight.dtype == torch.float32
                 or (weight.dtype == torch.bfloat16 and weight.is_contiguous()
                     and _aligned16(weight)))
            and (bias is None or (bias.device == h.device
                                  and bias.shape == weight.shape[:1])))


def _composite(h, weight, bias, labels, ignore_index, reduction):
    """F.linear + F.cross_entropy on h [N, K]: bf16 logits and an fp32 loss
    where the kernels would compute in bf16, the dtype of h otherwise."""
    if _bf16_compute(h):
        h, weight = h.to(torch.bfloat16), weight.to(torch.bfloat16)
        bias = None if bias is None else bias.to(torch.bfloat16)
    logits = F.linear(h, weight, bias)
    if logits.dtype == torch.bfloat16:
        logits = logits.float()
    return F.cross_entropy(logits, labels, ignore_index=ignore_index,
                           reduction=reduction)


_TUNER_PRIMED = set()


def _prime_gemm_tuner(h, weight, bias, labels, ignore_index):
    """A step under stream capture runs the composite (see above), whose
    three [N, V, K] GEMMs eager steps on the kernel path never launch. With
    TunableOp tuning on they would then be tuned at first sight inside the
    capture, where the tuner's timing loop invalidates it. So the first
    eager kernel-path call of a shape runs the composite once, forward and
    backward on detached operands, while tuning is on: the tuner has met
    the captured step's GEMMs before any capture, as it has when eager
    steps run the composite. Costs one composite call per shape, nothing
    when tuning is off."""
    key = (h.shape, weight.shape, weight.dtype, bias is not None, h.device)
    if key in _TUNER_PRIMED:
        return
    tunable = torch.cuda.tunable
    if not (tunable.is_enabled() and tunable.tuning_is_enabled()):
        return
    _TUNER_PRIMED.add(key)
    with torch.enable_grad():
        ops = [t.detach().requires_grad_(True) if t is not None else None
               for t in (h, weight, bias)]
        _composite(*ops, labels, ignore_index, "sum").backward()


class _LinearCEFn(torch.autograd.Function):
    """h [N, K] bf16, weight [V, K] bf16, bias [V] fp32 or None, labels [N]
    int64 -> (loss rows [N] fp32, mean over the kept rows). Saves the
    compacted rows and their log-sum-exp, never the logits."""

    @staticmethod
    def forward(ctx, h, weight, bias, labels, ignore_index, m_cap):
        ext = ops_api.ext()
        hc, rows, tgt, count = ext.lce_compact(h, labels, ignore_index, m_cap)
        loss, stats, lse2 = ext.lce_fwd(hc, weight, bias, rows, tgt, count,
                                        h.size(0))
        ctx.save_for_backward(hc, rows, tgt, lse2, count, weight, bias)
        ctx.n_rows = h.size(0)
        ctx.set_materialize_grads(False)
        return loss, stats[1]

    @staticmethod
    def backward(ctx, g_rows, g_mean):
        hc, rows, tgt, lse2, count, weight, bias = ctx.saved_tensors
        if g_rows is None and g_mean is None:
            return (None,) * 6
        if g_rows is not None:
            g_rows = g_rows.float().contiguous()
        if g_mean is not None:
            g_mean = g_mean.float().reshape(1)
        dz, db = ops_api.ext().lce_bwd(hc, weight, bias, rows, tgt, count,
                                       lse2, g_rows, g_mean)
        dz = dz[:, :weight.size(0)]     # the rows keep their 16-byte stride
        need = ctx.needs_input_grad
        dh = dw = None
        if need[0]:
            # pad rows of dz are zero, so are theirs of dHc: they all land in
            # one spare row past the end
            N = ctx.n_rows
            dh = hc.new_zeros(N + 1, hc.size(1))
            dh.index_copy_(0, torch.where(rows < 0, N, rows), dz @ weight)
            dh = dh[:N]
        if need[1]:
            dw = dz.t() @ hc
        return dh, dw, (db if need[2] else None), None, None, None


def _drop_past(labels, ignore_index, max_rows):
    """labels with every labelled position past the first max_rows set to
    ignore_index: what the kernels' compaction drops."""
    keep = labels != ignore_index
    return torch.where(keep & (keep.cumsum(0) > max_rows),
                       torch.full_like(labels, ignore_index), labels)


def fused_linear_cross_entropy(h, weight, bias, labels, ignore_index=-100,
                               reduction="mean", max_rows=None):
    """Cross-entropy of the logits h W^T + bias against `labels`, without
    the logits: h [..., K], weight [V, K] (fp32 or bf16), bias [V] or None,
    labels [...] int64 in [0, V) or ignore_index. On the kernel path any
    other label gives that row a NaN loss (the composite raises torch's
    device-side assert).

    reduction "mean" is over the labelled rows (NaN when there are none, as
    F.cross_entropy gives); "none" returns [N] fp32 rows, N the number of
    positions, with zeros in ignored rows.

    max_rows is the caller's static bound on the number of labelled rows
    (batch * max_predictions_per_seq for masked-LM data). It sizes the
    compacted operands, so the kernels and the backward GEMMs run on
    max_rows rows and not on N. Labelled rows past the first max_rows, in
    input order, are DROPPED exactly as if they were ignored. None: N."""
    if reduction not in ("mean", "none"):
        raise ValueError(f"reduction must be mean or none: {reduction}")
    K = h.size(-1)
    if labels.shape != h.shape[:-1]:
        raise ValueError("fused_linear_cross_entropy: h [..., K] and labels "
                         "[...] expected")
    N = labels.numel()
    m_cap = N if max_rows is None else max(1, min(int(max_rows), N))
    labels = labels.reshape(-1)
    if can_use_lce_kernels(h, weight, bias) and labels.device == h.device:
        h = h.reshape(N, K)
        _prime_gemm_tuner(h, weight, bias, labels, ignore_index)
        # recorded casts: the gradient reaches an fp32 (tied) table through
        # the cast's backward, as in fused_linear
        rows, mean = _LinearCEFn.apply(
            h.to(torch.bfloat16), weight.to(torch.bfloat16).contiguous(),
            None if bias is None else bias.float().contiguous(),
            labels.contiguous(), int(ignore_index), m_cap)
        return mean if reduction == "mean" else rows
    if m_cap < N:
        labels = _drop_past(labels, ignore_index, m_cap)
    return _composite(h.reshape(N, K), weight, bias, labels, ignore_index,
                      reduction)
