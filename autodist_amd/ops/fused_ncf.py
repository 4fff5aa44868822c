"""Fused NeuMF: the whole NCF model (four embedding gathers, the GMF product,
the MLP tower, the one-logit head and the BCE loss) as one forward and one
backward HIP kernel on the gfx950 fp32 matrix cores (ops/csrc/ncf_ops.hip),
plus a small fixed-order reduction of the dense gradients' partials.

    H_0  = [mlp_user[u], mlp_item[i]]
    H_l  = relu(H_{l-1} W_l^T + b_l)
    z    = w_head . [mf_user[u] * mf_item[i], H_L] + b_head
    loss = weight * (max(z, 0) - z y + log1p(exp(-|z|)))

Everything is fp32, as the module path without autocast is. The backward
writes one gradient row per sample for each of the four tables: for a table
built with sparse=True they are the values of an uncoalesced
torch.sparse_coo_tensor over the ids, the structure nn.Embedding(sparse=True)
produces, so the engine's sparse path serves it unchanged; otherwise the rows
are added in sorted order, without atomics, into a dense zero table.

`can_use_fused_neumf` says when a NeuMF module takes this path; everything
else (CPU, ShardedEmbedding tables, autocast, widths the kernels refuse)
keeps the module path. `AUTODIST_NCF=torch` forces the module path.
"""
import os

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from autodist_amd.ops import api as ops_api
from autodist_amd.ops.sampled_softmax import _scatter_rows


class _NeuMFFn(torch.autograd.Function):
    """(users, items, labels | None, weight | None, sparse flags, L, four
    tables, L weights, L biases, head weight, head bias) -> (logits [B],
    loss_rows [B] | None)."""

    @staticmethod
    def forward(ctx, users, items, labels, weight, sparse, n_layers, *params):
        ext = ops_api.ext()
        tables = list(params[:4])
        ws = list(params[4:4 + n_layers])
        bs = list(params[4 + n_layers:4 + 2 * n_layers])
        w_head, b_head = params[4 + 2 * n_layers:]
        save = any(ctx.needs_input_grad)
        logits, loss, acts = ext.neumf_fwd(users, items, tables, ws, bs,
                                           w_head, b_head, labels, weight,
                                           save)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(users, items, labels, weight, logits, acts,
                              *params)
        ctx.meta = (sparse, n_layers)
        return logits, (loss if labels is not None else None)

    @staticmethod
    @once_differentiable
    def backward(ctx, g_logits, g_loss):
        users, items, labels, weight, logits, acts, *params = ctx.saved_tensors
        sparse, L = ctx.meta
        n_in = 6 + len(params)
        if g_logits is None and g_loss is None:
            return (None,) * n_in
        tables = params[:4]
        ws, bs = params[4:4 + L], params[4 + L:4 + 2 * L]
        w_head, b_head = params[4 + 2 * L:]

        def rows(g):
            return None if g is None else g.float().contiguous()

        *d_rows, dense = ops_api.ext().neumf_bwd(
            users, items, list(tables), list(ws), list(bs), w_head, b_head,
            logits, acts, labels, weight, rows(g_logits), rows(g_loss))
        need = ctx.needs_input_grad[6:]
        grads = []
        for k, (table, d) in enumerate(zip(tables, d_rows)):
            ids = users if k % 2 == 0 else items
            if not need[k]:
                grads.append(None)
            elif sparse[k]:
                grads.append(torch.sparse_coo_tensor(ids[None], d,
                                                     table.shape))
            else:
                grads.append(_scatter_rows(table.size(0), ids, d))
        # dense: per layer dW then db, then the head's weight and bias
        dws, dbs, off = [], [], 0
        for w in ws:
            dws.append(dense[off:off + w.numel()].view_as(w))
            off += w.numel()
            dbs.append(dense[off:off + w.size(0)])
            off += w.size(0)
        d_head = [dense[off:off + w_head.numel()].view_as(w_head),
                  dense[off + w_head.numel():].view_as(b_head)]
        grads += [g if n else None
                  for g, n in zip(dws + dbs + d_head, need[4:])]
        return (None,) * 6 + tuple(grads)


def neumf_forward(users, items, tables, mlp, head, labels=None, weight=None):
    """NeuMF through the HIP kernels. users, items: int64 ids [B] on the GPU;
    tables: the nn.Embedding modules (mf_user, mf_item, mlp_user, mlp_item);
    mlp: nn.Sequential of Linear/ReLU pairs; head: nn.Linear to one logit;
    labels, weight: optional [B]. Returns (logits [B], loss_rows [B] | None).
    A shape the kernels do not serve raises; ask can_use_fused_neumf first."""
    linears = [m for m in mlp if isinstance(m, nn.Linear)]
    if labels is not None:
        labels = labels.float().contiguous()
    if weight is not None:
        if labels is None:
            raise ValueError("neumf_forward: weight needs labels")
        weight = weight.float().contiguous()
    params = ([t.weight for t in tables] + [m.weight for m in linears]
              + [m.bias for m in linears] + [head.weight, head.bias])
    return _NeuMFFn.apply(users.contiguous(), items.contiguous(), labels,
                          weight, tuple(bool(t.sparse) for t in tables),
                          len(linears), *params)


def _plain_f32(p):
    return (p is not None and p.is_cuda and p.dtype == torch.float32
            and p.is_contiguous() and p.data_ptr() % 16 == 0)


def can_use_fused_neumf(model, users):
    """True when the HIP kernels serve `model` (a models.ncf.NeuMF) on these
    ids: ids on the GPU and the extension loaded, autocast off, every
    parameter fp32 and contiguous, the four tables plain nn.Embedding without
    padding_idx, max_norm or scale_grad_by_freq, the MLP 1..NEUMF_MAX_LAYERS
    Linear(bias)/ReLU pairs, mf_dim and every MLP width a multiple of 8 in
    [8, NEUMF_MAX_WIDTH], and AUTODIST_NCF not "torch"."""
    if os.environ.get("AUTODIST_NCF") == "torch":
        return False
    if not (users.is_cuda and users.dtype == torch.int64 and users.dim() == 1
            and ops_api.has_gpu_ops()) or torch.is_autocast_enabled():
        return False
    ext = ops_api.ext()
    tables = (model.mf_user, model.mf_item, model.mlp_user, model.mlp_item)
    for t in tables:
        if type(t) is not nn.Embedding or t.padding_idx is not None \
                or t.max_norm is not None or t.scale_grad_by_freq \
                or not _plain_f32(t.weight):
            return False
    mods = list(model.mlp)
    linears = mods[0::2]
    if len(mods) % 2 or not 1 <= len(linears) <= ext.NEUMF_MAX_LAYERS \
            or any(type(m) is not nn.ReLU for m in mods[1::2]):
        return False
    widths = [model.mf_user.embedding_dim, 2 * model.mlp_user.embedding_dim]
    for m in linears:
        if type(m) is not nn.Linear or not _plain_f32(m.weight) \
                or not _plain_f32(m.bias):
            return False
        widths.append(m.out_features)
    if type(model.head) is not nn.Linear or model.head.out_features != 1 \
            or not _plain_f32(model.head.weight) \
            or not _plain_f32(model.head.bias):
        return False
    return (model.mf_item.embedding_dim == widths[0]
            and model.mlp_item.embedding_dim == model.mlp_user.embedding_dim
            and all(w % 8 == 0 and 8 <= w <= ext.NEUMF_MAX_WIDTH
                    for w in widths))
