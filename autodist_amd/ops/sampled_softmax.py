"""Sampled softmax loss: the loss the LM1B reference trains with
(tf.nn.sampled_softmax_loss, num_sampled candidates shared by the batch,
remove_accidental_hits=True, subtract_log_q=True).

    z0[n]   = h[n] . W[t_n] + b[t_n] - logq_true[n]
    z[n,s]  = h[n] . W[c_s] + b[c_s] - logq_samp[s],  -inf where c_s == t_n
    loss[n] = logsumexp(z0[n], z[n, 0..S)) - z0[n]

On the GPU with bf16 compute `sampled_softmax_loss` runs the ssm_* HIP kernels
(ops/csrc/ssm_ops.hip): one gather + cast pass over the S + N table rows, the
[N, S] logits on bf16 MFMA with the masking and the online log-sum-exp as
the epilogue (the logits are never stored), and in backward the recomputed
logits turned into dz [N, S_pad] bf16, dz0 and the sampled bias gradient.

What stays on hipBLASLt through torch, as in fused_lstm.py: dH = dz Wg,
dWg = dz^T H (one GEMM each) and the row-wise dz0 terms (dz0 * Wt into dH,
dz0 * h into the target rows' gradient).

The weight gradient touches at most S + N rows. With sparse_grad=True it is
an uncoalesced torch.sparse_coo_tensor over cat(sampled, targets), which the
engine's sparse path serves; otherwise the rows are added, in sorted order
and without atomics, into a dense zero table. The bias gradient is always dense ([V] floats).

Everything else (CPU, fp32 / fp64 compute, a shape the kernels refuse) runs
the plain torch composite of the formulas. `AUTODIST_SAMPLED_SOFTMAX=torch`
forces the composite.
"""
import math
import os

import torch
import torch.nn.functional as F

from autodist_amd.ops import api as ops_api


class LogUniformSampler:
    """Log-uniform (Zipfian) candidate sampler over [0, range_max), drawn
    WITH replacement on the device: k = floor(exp(u ln(range_max + 1))) - 1,
    u uniform in [0, 1). The expected count of class k among num_sampled
    draws is Q(k) = num_sampled (ln(k + 2) - ln(k + 1)) / ln(range_max + 1).

    This is TF's log_uniform_candidate_sampler with unique=False. The
    reference's default sampler is the unique one (it rejects repeats and
    corrects Q for the number of tries); here a class drawn twice is two
    separate columns of the loss, each with its own -log Q correction.

    Shapes are fixed and nothing is read back to the host, so a step that
    samples stays capturable."""

    def __init__(self, range_max, num_sampled, seed=0):
        assert range_max >= 1 and num_sampled >= 1
        self.range_max = int(range_max)
        self.num_sampled = int(num_sampled)
        self.seed = int(seed)
        self._log_range = math.log(self.range_max + 1.0)
        self._gens = {}

    def _generator(self, device):
        device = torch.device(device)
        gen = self._gens.get(device)
        if gen is None:
            gen = torch.Generator(device=device).manual_seed(self.seed)
            self._gens[device] = gen
        return gen

    def _logq(self, ids):
        k = ids.double()
        p = torch.log1p(1.0 / (k + 1.0)) / self._log_range
        return torch.log(self.num_sampled * p).float()

    def sample(self, device="cpu"):
        """(sampled [num_sampled] int64, logq_samp [num_sampled] fp32)."""
        u = torch.rand(self.num_sampled, dtype=torch.float64, device=device,
                       generator=self._generator(device))
        k = torch.exp(u * self._log_range).floor().long() - 1
        k = k.clamp_(0, self.range_max - 1)
        return k, self._logq(k)

    def logq_true(self, targets):
        """log Q of the target classes, fp32, shaped like `targets`."""
        return self._logq(targets)


def _bf16_compute(h):
    return h.is_cuda and (h.dtype == torch.bfloat16
                          or torch.is_autocast_enabled())


def can_use_ssm_kernels(h, weight, bias):
    """True when the HIP kernels serve this call: h [N, P] on the GPU with
    bf16 compute (a bf16 h, or autocast on), an fp32 or bf16 contiguous
    table, P a multiple of 32 up to SSM_MAX_P, the extension loaded and
    AUTODIST_SAMPLED_SOFTMAX not "torch"."""
    if os.environ.get("AUTODIST_SAMPLED_SOFTMAX") == "torch":
        return False
    if not (_bf16_compute(h) and ops_api.has_gpu_ops()):
        return False
    P = h.size(1)
    return (h.size(0) >= 1 and P % 32 == 0
            and 32 <= P <= ops_api.ext().SSM_MAX_P
            and weight.dtype in (torch.float32, torch.bfloat16)
            and weight.is_contiguous()
            and (bias is None or bias.dtype == torch.float32))


def _scatter_rows(rows, ids, values):
    """zeros(rows, ...) with values[i] added into row ids[i]. index_put_
    with accumulate sorts the ids and adds each row's values in order, so
    repeated ids give the same bits every run (index_add_ uses atomics)."""
    out = values.new_zeros((rows,) + tuple(values.shape[1:]))
    return out.index_put_((ids,), values, accumulate=True)


class _SampledSoftmaxFn(torch.autograd.Function):
    """h [N, P] bf16, table [V, P] fp32 or bf16, bias [V] fp32 or None ->
    loss rows [N] fp32."""

    @staticmethod
    def forward(ctx, h, weight, bias, targets, sampled, logq_true, logq_samp,
                sparse_grad):
        ext = ops_api.ext()
        wg, wt, off, off0 = ext.ssm_prep(weight, bias, sampled, targets,
                                         logq_samp, logq_true)
        loss, lse2, z0 = ext.ssm_fwd(h, wg, wt, off, off0, sampled, targets)
        ctx.save_for_backward(h, wg, wt, sampled, targets, lse2, z0, off)
        ctx.table = (weight.size(0), weight.dtype, sparse_grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        ext = ops_api.ext()
        h, wg, wt, sampled, targets, lse2, z0, off = ctx.saved_tensors
        V, w_dtype, sparse_grad = ctx.table
        S = sampled.numel()
        dz, dz0, db_samp = ext.ssm_bwd(h, wg, off, sampled, targets, lse2,
                                       z0, g.float().contiguous())
        need = ctx.needs_input_grad
        dh = dw = db = None
        if need[0]:
            dh = torch.addcmul((dz @ wg).float(), dz0[:, None],
                               wt.float()).to(h.dtype)
        if need[1]:
            ids = torch.cat([sampled, targets])[None]
            vals = torch.cat([(dz.t() @ h)[:S].float(),
                              dz0[:, None] * h.float()])
            size = (V, h.size(1))
            if sparse_grad:
                dw = torch.sparse_coo_tensor(ids, vals.to(w_dtype), size)
            else:
                dw = _scatter_rows(V, ids[0], vals).to(w_dtype)
        if need[2]:
            db = _scatter_rows(V, torch.cat([sampled, targets]),
                               torch.cat([db_samp, dz0]))
        return dh, dw, db, None, None, None, None, None


def _composite(h, weight, bias, targets, sampled, logq_true, logq_samp,
               sparse_grad):
    """The formulas in plain torch. Operands are bf16 where the kernels
    would be (GPU with a bf16 h or autocast), the dtype of h otherwise;
    offsets, masking and the log-sum-exp run in fp32 (fp64 for an fp64 h)."""
    cd = torch.bfloat16 if _bf16_compute(h) else h.dtype
    acc = torch.float64 if cd == torch.float64 else torch.float32
    hc = h.to(cd)
    wg = F.embedding(sampled, weight, sparse=sparse_grad).to(cd)
    wt = F.embedding(targets, weight, sparse=sparse_grad).to(cd)
    z = (hc @ wg.t()).to(acc)
    z0 = (hc.to(acc) * wt.to(acc)).sum(-1)
    if bias is not None:
        z = z + bias.index_select(0, sampled).to(acc)
        z0 = z0 + bias.index_select(0, targets).to(acc)
    z = z - logq_samp.to(acc)
    z0 = z0 - logq_true.to(acc)
    z = z.masked_fill(sampled[None, :] == targets[:, None], float("-inf"))
    lse = torch.logsumexp(torch.cat([z0[:, None], z], 1), 1)
    return lse - z0


def sampled_softmax_loss(h, weight, bias, targets, sampled, logq_true,
                         logq_samp, reduction="mean", sparse_grad=False):
    """Sampled softmax loss of h [N, P] against table `weight` [V, P] and
    optional `bias` [V]: targets [N] and the shared candidates sampled [S]
    are int64 ids in [0, V) (the caller's contract, as for gather_rows);
    duplicates in `sampled` are separate columns. logq_true [N] and
    logq_samp [S] are the log expected counts the sampler returns.
    reduction: "mean", "sum" or "none" (fp32 loss rows [N])."""
    if reduction not in ("mean", "sum", "none"):
        raise ValueError(f"reduction must be mean, sum or none: {reduction}")
    if h.dim() != 2 or targets.shape != h.shape[:1] or sampled.dim() != 1 \
            or sampled.numel() < 1:
        raise ValueError("sampled_softmax_loss: h [N, P], targets [N] and a "
                         "non-empty sampled [S] expected")
    logq_true, logq_samp = logq_true.float(), logq_samp.float()
    if can_use_ssm_kernels(h, weight, bias):
        rows = _SampledSoftmaxFn.apply(
            h.to(torch.bfloat16).contiguous(), weight, bias, targets.contiguous(),
            sampled.contiguous(), logq_true.contiguous(),
            logq_samp.contiguous(), sparse_grad)
    else:
        rows = _composite(h, weight, bias, targets, sampled, logq_true,
                          logq_samp, sparse_grad)
    if reduction == "none":
        return rows
    return rows.mean() if reduction == "mean" else rows.sum()
