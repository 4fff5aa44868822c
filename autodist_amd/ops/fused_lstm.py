"""Projected LSTM (nn.LSTM with proj_size) on the bf16 matrix cores.

`fused_lstmp(x, lstm, state)` runs an `nn.LSTM` module's parameters through
the lstmp_cell_* HIP kernels (ops/csrc/lstm_ops.hip): per time step one
kernel does the recurrent GEMM h_{t-1} W_hh^T for all four gates of a tile
of hidden units and, as its epilogue, the bias add, the activations, the
cell update and o * tanh(c). The module is only the parameter holder, so
names, shapes, state dicts and checkpoints are those of nn.LSTM.

What stays on hipBLASLt through torch, as in FusedLinear: the input
projection X W_ih^T for all time steps at once, per step the projection
h_t = hc_t W_hr^T (a reduction over the full H, across the kernel's
workgroups) and in backward dh_{t-1} += dgates_t W_hh; after the time loop
ONE GEMM each for dW_ih, dW_hh, dW_hr and dX over the stacked [T*B, .]
buffers. The bias gradient is the col_sum kernel on the stacked dgates.

Numerics: operands and the stored h / gates / dgates are bf16, every
accumulation, the gate math and the cell state c are fp32. Saved for
backward per layer: x, the activated gates [T, B, 4H] bf16, hc [T, B, H]
bf16, c [T+1, B, H] fp32, h [T+1, B, P] bf16.

`AUTODIST_LSTM=torch` sends every call to the stock module.
"""
import os

import torch
import torch.nn.functional as F

from autodist_amd.ops import api as ops_api


def _shapes_ok(lstm):
    e = ops_api.ext()
    P, H = lstm.proj_size, lstm.hidden_size
    return (P % 32 == 0 and 32 <= P <= e.LSTMP_MAX_P and H % 16 == 0
            and lstm.input_size % 8 == 0)


def can_use_fused_lstmp(x, lstm):
    """True when fused_lstmp serves this (input, module) pair: a
    unidirectional batch_first nn.LSTM with biases and a projection, P a
    multiple of 32 (at most LSTMP_MAX_P), H a multiple of 16, the input size
    a multiple of 8 (16-byte bf16 rows), a 3-D x on the GPU, the extension
    loaded and AUTODIST_LSTM not "torch"."""
    return (os.environ.get("AUTODIST_LSTM") != "torch"
            and isinstance(lstm, torch.nn.LSTM)
            and not lstm.bidirectional and lstm.batch_first and lstm.bias
            and lstm.proj_size > 0
            and x.is_cuda and x.dim() == 3 and x.size(0) > 0 and x.size(1) > 0
            and ops_api.has_gpu_ops() and _shapes_ok(lstm))


class _LSTMPLayerFn(torch.autograd.Function):
    """One layer over all time steps. x [B, T, E], w_ih [4H, E], w_hh
    [4H, P], w_hr [P, H], h0 [B, P] in bf16; bias [4H] (b_ih + b_hh) and c0
    [B, H] in fp32 -> out [B, T, P] bf16, h_n [B, P] bf16, c_n [B, H] fp32.
    Buffers are time-major inside, so each step's slice is contiguous."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, w_hr, bias, h0, c0):
        ext = ops_api.ext()
        ctx.set_materialize_grads(False)
        B, T, E = x.shape
        H, P = w_hr.shape[1], w_hr.shape[0]
        x_tm = x.transpose(0, 1).contiguous()
        gx = (x_tm.view(T * B, E) @ w_ih.t()).view(T, B, 4 * H)
        w_hh = w_hh.contiguous()
        w_hr = w_hr.contiguous()
        w_hr_t = w_hr.t()
        h = torch.empty(T + 1, B, P, dtype=torch.bfloat16, device=x.device)
        c = torch.empty(T + 1, B, H, dtype=torch.float32, device=x.device)
        hc = torch.empty(T, B, H, dtype=torch.bfloat16, device=x.device)
        gates = torch.empty(T, B, 4 * H, dtype=torch.bfloat16,
                            device=x.device)
        h[0].copy_(h0)
        c[0].copy_(c0)
        for t in range(T):
            ext.lstmp_cell_fwd(gx[t], h[t], w_hh, bias, c[t], c[t + 1],
                               hc[t], gates[t])
            torch.mm(hc[t], w_hr_t, out=h[t + 1])
        ctx.save_for_backward(x_tm, w_ih, w_hh, w_hr, h, c, hc, gates)
        return h[1:].transpose(0, 1), h[T].clone(), c[T].clone()

    @staticmethod
    def backward(ctx, d_out, d_hn, d_cn):
        ext = ops_api.ext()
        x_tm, w_ih, w_hh, w_hr, h, c, hc, gates = ctx.saved_tensors
        T, B, E = x_tm.shape
        H, P = w_hr.shape[1], w_hr.shape[0]
        dev = x_tm.device
        if d_out is None:
            d_out = torch.zeros(B, T, P, dtype=torch.bfloat16, device=dev)
        d_out = d_out.to(torch.bfloat16)
        dh = torch.empty(T, B, P, dtype=torch.bfloat16, device=dev)
        dgates = torch.empty(T, B, 4 * H, dtype=torch.bfloat16, device=dev)
        dc = torch.empty(B, H, dtype=torch.float32, device=dev)
        dc_next = None
        if d_cn is not None:
            dc.copy_(d_cn)
            dc_next = dc
        dh_rec = d_hn.to(torch.bfloat16) if d_hn is not None else None
        for t in range(T - 1, -1, -1):
            # gradient from the layer above plus the recurrent one
            if dh_rec is None:
                dh[t].copy_(d_out[:, t])
            else:
                torch.add(d_out[:, t], dh_rec, out=dh[t])
            ext.lstmp_cell_bwd(dh[t], w_hr, gates[t], c[t + 1], c[t],
                               dc_next, dgates[t], dc)
            dc_next = dc
            dh_rec = dgates[t] @ w_hh
        dg2 = dgates.view(T * B, 4 * H)
        need = ctx.needs_input_grad
        dx = (dg2 @ w_ih).view(T, B, E).transpose(0, 1) if need[0] else None
        dw_ih = dg2.t() @ x_tm.view(T * B, E) if need[1] else None
        dw_hh = dg2.t() @ h[:T].view(T * B, P) if need[2] else None
        dw_hr = (dh.view(T * B, P).t() @ hc.view(T * B, H)
                 if need[3] else None)
        dbias = ext.col_sum(dg2) if need[4] else None
        return (dx, dw_ih, dw_hh, dw_hr, dbias,
                dh_rec if need[5] else None, dc if need[6] else None)


def fused_lstmp(x, lstm, state=None):
    """nn.LSTM forward for a module that `can_use_fused_lstmp` accepts:
    returns (out [B, T, P], (h_n [layers, B, P], c_n [layers, B, H])) as
    the module does, with out and h_n in bf16 and c_n in fp32. `state` is
    the module's (h_0, c_0) or None for zeros.

    Weights are cast to bf16 once per call by recorded casts, so gradients
    reach the fp32 parameters in fp32. In training, inter-layer dropout is
    F.dropout on each layer's output but the last: the distribution
    nn.LSTM uses, drawn from a different RNG stream, so a seeded run does
    not reproduce the stock module's masks."""
    if not can_use_fused_lstmp(x, lstm):
        raise RuntimeError(
            "fused_lstmp: unsupported module, input or build (see "
            "can_use_fused_lstmp); call the nn.LSTM module instead")
    B = x.size(0)
    bf = torch.bfloat16
    inp = x.to(bf)
    h_n, c_n = [], []
    for layer in range(lstm.num_layers):
        w_ih = getattr(lstm, f"weight_ih_l{layer}").to(bf)
        w_hh = getattr(lstm, f"weight_hh_l{layer}").to(bf)
        w_hr = getattr(lstm, f"weight_hr_l{layer}").to(bf)
        bias = (getattr(lstm, f"bias_ih_l{layer}").float()
                + getattr(lstm, f"bias_hh_l{layer}").float())
        if state is None:
            h0 = torch.zeros(B, lstm.proj_size, dtype=bf, device=x.device)
            c0 = torch.zeros(B, lstm.hidden_size, dtype=torch.float32,
                             device=x.device)
        else:
            h0, c0 = state[0][layer].to(bf), state[1][layer].float()
        inp, h_l, c_l = _LSTMPLayerFn.apply(inp, w_ih, w_hh, w_hr, bias,
                                            h0, c0)
        h_n.append(h_l)
        c_n.append(c_l)
        if lstm.dropout > 0 and lstm.training and layer + 1 < lstm.num_layers:
            inp = F.dropout(inp, lstm.dropout, True)
    return inp, (torch.stack(h_n), torch.stack(c_n))
