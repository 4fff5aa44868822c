"""Fused LSTMP: lstmp_cell_fwd / lstmp_cell_bwd against float64 on the
bf16-rounded operands, exact saturation / gate-order cases, and the public
path through LM1BModel and fused_lstmp.

Error model of the single-step tests (u = 2^-24, K = P terms per dot
product, TR the activation's absolute error):

  pre-activation  e_pre = (K + 2) u (|gx| + |bias| + sum_k |h_k w_k|)
  sigmoid gates   e = e_pre / 4 + TR      (|sigma'| <= 1/4)
  tanh gate       e = e_pre + TR          (|tanh'| <= 1)
  c_t             |c_prev| e_f + e_i + e_g + 4u (|f c_prev| + |i g|)
  hc_t            e_o + e_c + TR + 4u
  dhc             e_dhc = K u sum_k |dh_k w_hr[k, j]|
  dc              e_dc = e_dhc + |dhc| (2 TR + 4u) + 4u (|dc| + |dc_next|)
  dc_prev         e_dc + 4u |ref|
  d{i,f,g}        e_dc |factor| + 8u |ref|, factor = dgate / dc
  do              (e_dhc + |dhc| TR) o (1 - o) + 8u |ref|

bf16-stored outputs (gates, hc_t, dgates) add 2^-7 |ref|. TR = 2^-23: the
kernel's formulas 1 / (1 + exp(-x)) and copysign((1 - e) / (1 + e), x), e =
exp(-2|x|), evaluated in fp32 on the CPU over 10^7 points of [-30, 30],
measure 1.49 * 2^-24 (sigmoid) and 1.50 * 2^-24 (tanh) against float64; the
device exp is good to 1 ulp where the host's is to 0.5, which adds at most
0.5 * 2^-24 to either."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
BF16 = 2.0 ** -7
TR = 2.0 ** -23


@pytest.fixture
def ext():
    from autodist_amd.ops import api
    if not api.has_gpu_ops():
        pytest.skip("no GPU ops")
    return api.ext()


def _within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    print(f"{name}: max err {err.max().item():.3e}, "
          f"max err / bound {(err / tol.clamp_min(1e-300)).max().item():.3f}")
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, "
        f"max err {err.max().item():.3e}")


def _bf(*shape, g, scale=1.0):
    return (torch.randn(*shape, generator=g, device="cuda") * scale).bfloat16()


def _cell_fwd(ext, gx, h, w_hh, bias, c_prev):
    B, H = c_prev.shape
    c = torch.empty_like(c_prev)
    hc = torch.empty(B, H, dtype=torch.bfloat16, device="cuda")
    gates = torch.empty(B, 4 * H, dtype=torch.bfloat16, device="cuda")
    ext.lstmp_cell_fwd(gx, h, w_hh, bias, c_prev, c, hc, gates)
    return c, hc, gates


@pytest.mark.parametrize("H", [16, "tile+16"])
@pytest.mark.parametrize("P", [32, 96])
@pytest.mark.parametrize("B", [1, "tile+3"])
def test_lstmp_cell_vs_float64(ext, B, P, H):
    B = ext.LSTMP_TILE_B + 3 if B == "tile+3" else B
    H = ext.LSTMP_TILE_H + 16 if H == "tile+16" else H
    g = torch.Generator(device="cuda").manual_seed(B * 1000 + P + H)
    gx = _bf(B, 3, 4 * H, g=g, scale=2.0)[:, 1]       # row-strided slice
    h, w_hh = _bf(B, P, g=g), _bf(4 * H, P, g=g, scale=0.3)
    bias = torch.randn(4 * H, generator=g, device="cuda")
    c_prev = torch.randn(B, H, generator=g, device="cuda") * 2
    c, hc, gates = _cell_fwd(ext, gx, h, w_hh, bias, c_prev)

    hd, wd, cpd = h.double(), w_hh.double(), c_prev.double()
    pre = gx.double() + bias.double() + hd @ wd.t()
    e_pre = (P + 2) * U * (gx.double().abs() + bias.double().abs()
                           + hd.abs() @ wd.abs().t())
    i, f, gg, o = pre.view(B, 4, H).unbind(1)
    i, f, gg, o = i.sigmoid(), f.sigmoid(), gg.tanh(), o.sigmoid()
    e_i, e_f, e_g, e_o = e_pre.view(B, 4, H).unbind(1)
    e_i, e_f, e_g, e_o = e_i / 4 + TR, e_f / 4 + TR, e_g + TR, e_o / 4 + TR
    c_ref = f * cpd + i * gg
    e_c = cpd.abs() * e_f + e_i + e_g + 4 * U * ((f * cpd).abs()
                                                 + (i * gg).abs())
    g_ref = torch.cat([i, f, gg, o], 1)
    _within("c_t", c, c_ref, e_c)
    _within("gates", gates, g_ref,
            torch.cat([e_i, e_f, e_g, e_o], 1) + BF16 * g_ref.abs())
    hc_ref = o * c_ref.tanh()
    _within("hc_t", hc, hc_ref, e_o + e_c + TR + 4 * U + BF16 * hc_ref.abs())

    # backward step on the kernel's own saved tensors
    dh, w_hr = _bf(B, 3, P, g=g)[:, 2], _bf(P, H, g=g, scale=0.3)
    dc_next = torch.randn(B, H, generator=g, device="cuda")
    dgates = torch.zeros(B, 3, 4 * H, dtype=torch.bfloat16, device="cuda")
    dc_prev = torch.empty(B, H, device="cuda")
    ext.lstmp_cell_bwd(dh, w_hr, gates, c, c_prev, dc_next, dgates[:, 1],
                       dc_prev)
    assert not dgates[:, 0].any() and not dgates[:, 2].any()
    i, f, gg, o = gates.double().view(B, 4, H).unbind(1)
    dhc = dh.double() @ w_hr.double()
    e_dhc = P * U * (dh.double().abs() @ w_hr.double().abs())
    tc = c.double().tanh()
    dc = dhc * o * (1 - tc * tc) + dc_next.double()
    e_dc = (e_dhc + dhc.abs() * (2 * TR + 4 * U)
            + 4 * U * (dc.abs() + dc_next.double().abs()))
    _within("dc_prev", dc_prev, dc * f, e_dc + 4 * U * (dc * f).abs())
    fac = torch.cat([gg * i * (1 - i), cpd * f * (1 - f), i * (1 - gg * gg)],
                    1)
    d_ref = torch.cat([dc.repeat(1, 3) * fac, dhc * tc * o * (1 - o)], 1)
    e_d = torch.cat([e_dc.repeat(1, 3) * fac.abs(),
                     (e_dhc + dhc.abs() * TR) * o * (1 - o)], 1)
    _within("dgates", dgates[:, 1], d_ref, e_d + (8 * U + BF16) * d_ref.abs())
    # dc_next = None is a zero dc_next
    ext.lstmp_cell_bwd(dh, w_hr, gates, c, c_prev, None, dgates[:, 1], dc_prev)
    dc0 = dhc * o * (1 - tc * tc)
    _within("dc_prev, no dc_next", dc_prev, dc0 * f,
            e_dc + 4 * U * (dc0 * f).abs())


@pytest.mark.parametrize("gate", [0, 1, 2, 3], ids=list("ifgo"))
def test_lstmp_cell_saturation_and_gate_order(ext, gate):
    """w_hh = 0, so the pre-activations are gx. In fp32 sigmoid(80) == 1 and
    sigmoid(-80) < 2^-100 (checked on the CPU formula first), which pins
    each gate's row block exactly; +-120 overflows a naive tanh / exp."""
    one = torch.tensor(80.0)
    assert (1 / (1 + torch.exp(-one))).item() == 1.0
    assert (1 / (1 + torch.exp(one))).item() < 2.0 ** -100
    B, P, H = 3, 32, ext.LSTMP_TILE_H + 16
    g = torch.Generator(device="cuda").manual_seed(gate)
    h, w_hh = _bf(B, P, g=g), torch.zeros(4 * H, P, device="cuda").bfloat16()
    bias = torch.zeros(4 * H, device="cuda")
    c_prev = torch.randn(B, H, generator=g, device="cuda")
    c_prev = torch.where(c_prev.abs() < 2.0 ** -10, 1.0, c_prev)
    for v in (120.0, -120.0):
        gx = _bf(B, 4, H, g=g)
        gx[:, gate] = v
        for out in _cell_fwd(ext, gx.view(B, 4 * H), h, w_hh, bias, c_prev):
            assert torch.isfinite(out.float()).all()
    gx = _bf(B, 4, H, g=g)
    if gate in (0, 1):          # i closed, f open: the cell is carried
        gx[:, 0], gx[:, 1] = -80.0, 80.0
    elif gate == 2:             # i open, f closed, g = tanh(80) = 1
        gx[:, 0], gx[:, 1], gx[:, 2] = 80.0, -80.0, 80.0
    else:
        gx[:, 3] = -80.0
    c, hc, _ = _cell_fwd(ext, gx.view(B, 4 * H), h, w_hh, bias, c_prev)
    if gate in (0, 1):
        assert torch.equal(c, c_prev)
    elif gate == 2:
        assert torch.equal(c, torch.ones_like(c))
    else:
        assert (hc.float().abs() < 1e-30).all()


def _model(ext):
    from autodist_amd.models.lm1b import LM1BModel
    torch.manual_seed(3)
    model = LM1BModel(vocab_size=64, emb_dim=32, hidden=ext.LSTMP_TILE_H + 16,
                      proj=32, layers=2, dropout=0.0).cuda()
    with torch.no_grad():      # bf16-representable parameters
        for p in model.parameters():
            p.copy_(p.bfloat16())
    return model


@pytest.mark.parametrize("switch", [None, "torch"])
def test_lm1b_hidden_dispatch(ext, monkeypatch, switch):
    if switch:
        monkeypatch.setenv("AUTODIST_LSTM", switch)
    model = _model(ext).eval()
    tokens = torch.randint(0, 64, (5, 3), device="cuda")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        h, _ = model._hidden(tokens)
    fused = type(h.grad_fn).__name__ == "_LSTMPLayerFnBackward"
    assert fused == (switch is None)


@pytest.mark.parametrize("T,with_state", [(1, False), (3, False), (3, True)])
def test_fused_lstmp_public_path(ext, T, with_state):
    """out, h_n, c_n, dX and every LSTM parameter gradient against the
    float64 nn.LSTM on the same (bf16-representable) weights and inputs.
    Tolerance per tensor: twice the max-abs error of stock nn.LSTM under
    bf16 autocast at the same inputs against the same reference."""
    from autodist_amd.ops.fused_lstm import fused_lstmp
    model = _model(ext)
    lstm = model.lstm
    B, P, H = 5, lstm.proj_size, lstm.hidden_size
    g = torch.Generator(device="cuda").manual_seed(T)
    x0 = _bf(B, T, 32, g=g).float()
    state = None
    if with_state:
        state = (_bf(2, B, P, g=g).float(), _bf(2, B, H, g=g).float())
    w_out, w_h, w_c = (torch.randn(*s, generator=g, device="cuda")
                       for s in [(B, T, P), (2, B, P), (2, B, H)])

    def run(fn, mod, dev, dtype):
        mod.zero_grad(set_to_none=True)
        x = x0.to(dev, dtype).clone().requires_grad_(True)
        st = state and tuple(s.to(dev, dtype) for s in state)
        with torch.autocast("cuda", dtype=torch.bfloat16,
                            enabled=dtype == torch.float32):
            out, (h_n, c_n) = fn(x, mod, st)
        loss = ((out.double() * w_out.to(dev)).sum()
                + (h_n.double() * w_h.to(dev)).sum()
                + (c_n.double() * w_c.to(dev)).sum())
        loss.backward()
        res = {"out": out, "h_n": h_n, "c_n": c_n, "dX": x.grad}
        res.update({"d" + n: p.grad for n, p in mod.named_parameters()})
        return {k: v.detach().double().cpu() for k, v in res.items()}

    got = run(fused_lstmp, lstm, "cuda", torch.float32)
    stock = run(lambda x, m, s: m(x, s), lstm, "cuda", torch.float32)
    ref = run(lambda x, m, s: m(x, s), copy.deepcopy(lstm).cpu().double(),
              "cpu", torch.float64)
    worst = []
    for k in ref:
        e_f = (got[k] - ref[k]).abs().max().item()
        e_s = (stock[k] - ref[k]).abs().max().item()
        print(f"{k}: fused {e_f:.3e} stock-bf16 {e_s:.3e}")
        if not e_f <= 2 * e_s:
            worst.append((k, e_f, e_s))
    assert not worst, f"fused error above 2x stock bf16 nn.LSTM: {worst}"
