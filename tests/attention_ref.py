"""References, error model and input builders for the MFMA attention tests.

Shared by tests/test_attention_model.py (CPU) and
tests/test_attention_geometry_gpu.py / tests/test_attention_gpu.py (GPU).
Plain torch + numpy, device-agnostic, needs no GPU and no extension.

What the kernels compute (csrc/attention.hip, csrc/attention_bwd.hip), for
bf16 q, k, v, dO of shape [B, H, S, D], an additive fp32 key mask [B, S], a
keep-mask keep[b, h, q, k] in {0, 1} and rk = 1 / (1 - p):

    P  = softmax(Q K^T * scale + mask)        Pd = P o keep * rk
    O  = Pd V
    delta = rowsum(dO o o_in)                 (o_in: the bf16 O given to bwd)
    dP = keep * rk o (dO V^T)                 dS = P o (dP - delta) * scale
    dQ = dS K      dK = dS^T Q      dV = Pd^T dO

`reference` evaluates exactly these formulas in float64 on the bf16 inputs.
delta is taken from the tensor the backward kernel was handed (its own
forward's rounded output), as the LayerNorm tests take the kernel's own
u / mean / rstd: the rounding of O is an input of the backward, not an error
of it.

Error model (first order; nothing here is fitted to what a kernel returns).
u = 2^-9 stands for one round-to-nearest-even bf16 store: half its
worst-case relative error (2^-8, an 8-bit significand) and about its
typical size; sums of many such errors stay well below the sum of their
worst cases, a few dominant terms do not, and the measured margin k (below)
is what covers that. The kernels work in the exp2 domain:
logit2 = (Q K^T * scale + mask) * log2(e), m_i = max_j logit2_ij,
p_ij = exp2(logit2_ij - m_i) / l_i, everything before the bf16 store of p
in fp32. The fp32 scale-multiply, mask add and
subtraction of m leave an absolute error of a few 2^-24 * (|logit2| + |m|)
in the exponent, and exp2 itself and the division a few more ulps, hence a
relative error of p_ij of

    e_ij = 2^-22 * (|logit2_ij| + |m_i| + 8)

e is per element and is used only multiplied by P_ij: a key masked with
-30000 or -inf has P = 0 exactly, so its huge |logit2| never enters a bound
(a global max|logit2| would inflate every bound 8x). e is set to 0 where
P = 0, which also keeps inf * 0 out of the -inf case. Then

    tol_O  = sum_k (u + e) Pd |V|   + u |O|
    tol_dV = sum_q (u + e) Pd |dO|  + u |dV|
    a_dS   = u |dS| + scale * P o ( e o (|dP| + |delta|)
                 + 2^-21 * (keep * rk o (|dO| |V|^T) + rowsum|dO o o_in|) )
    tol_dQ = a_dS |K|   + u |dQ|
    tol_dK = a_dS^T |Q| + u |dK|

per element: (u + e) Pd is the error of the bf16-staged probability, the
trailing u|.| the bf16 store of the output; a_dS is the error of the
bf16-staged dS: its own store, the relative error e of P, and the fp32
accumulation error (2^-21 of the sum of |terms|) of dP and delta. The fp32
MFMA accumulation of the outer products (<= 352 terms * 2^-24) is an order
below u and is left to the margin k.

`emulate` repeats the computation in fp32 torch with bf16 casts at the
kernels' own rounding points, read off the kernel sources:
  forward   64-key tiles, running max m and sum l in fp32; the UNnormalised
            exp2(logit2 - m_running) o keep is what is stored bf16 and fed
            to the P V product; l sums the undropped fp32 values;
            O = acc / l * rk -> bf16.
  backward  p = exp2(logit2 - m) / l in fp32 (m, l of the finished row);
            dV uses the normalised p o keep * rk -> bf16; dS -> bf16 (the
            scale folded in before the store); dQ, dK, dV -> bf16.
It shares the model's rounding points but not the MFMA accumulation order
nor v_exp_f32's last-ulp behaviour; tests/test_attention_model.py measures
its worst err / tol and derives the one margin k from it.

`drop_keep` is an independent numpy replica of the kernels' counter hash and
threshold, so the `attn_dropmask` debug kernel (which shares the hash code
with the kernels it is used to check) is itself checked.
"""
import math
from types import SimpleNamespace

import numpy as np
import torch

U_BF16 = 2.0 ** -9
LOG2E = math.log2(math.e)
LOG2E_F32 = float(np.float32(1.4426950408889634))
# measured by tests/test_attention_model.py (see its header): the emulation's
# worst err / tol over all CASES is R_EMU, and K_MARGIN = ceil(2 * R_EMU)
K_MARGIN = 4
OUTPUTS = ("O", "dQ", "dK", "dV")


def _f32(x):
    return float(np.float32(x))


def _rkeep(p_drop):
    """1 / (1 - p) as the kernels form it, in fp32."""
    if not p_drop > 0.0:
        return 1.0
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))


# ---------------------------------------------------------------- reference
def reference(q, k, v, dout, scale, add_mask=None, keep=None, p_drop=0.0,
              o_in=None):
    """float64 forward + FA2 backward on the bf16 inputs, with the
    per-element first-order bounds of the module header.
    Returns a namespace with .out[name] and .tol[name], name in OUTPUTS."""
    scale = _f32(scale)
    rk = _rkeep(p_drop)
    Q, K, V, dO = (t.double() for t in (q, k, v, dout))
    logit2 = (Q @ K.transpose(-1, -2)) * (scale * LOG2E)
    if add_mask is not None:
        logit2 = logit2 + (add_mask.double() * LOG2E)[:, None, None, :]
    m = logit2.amax(-1, keepdim=True)
    P = torch.exp2(logit2 - m)
    P = P / P.sum(-1, keepdim=True)
    kf = keep.double() * rk if keep is not None else torch.ones_like(P)
    Pd = P * kf
    O = Pd @ V
    oi = O if o_in is None else o_in.double()
    delta = (dO * oi).sum(-1, keepdim=True)
    dP = kf * (dO @ V.transpose(-1, -2))
    dS = P * (dP - delta) * scale
    dQ = dS @ K
    dK = dS.transpose(-1, -2) @ Q
    dV = Pd.transpose(-1, -2) @ dO

    u = U_BF16
    e = 2.0 ** -22 * (logit2.abs() + m.abs() + 8.0)
    e = torch.where(P > 0, e, torch.zeros_like(e))
    pe = (u + e) * Pd
    tol_O = pe @ V.abs() + u * O.abs()
    tol_dV = pe.transpose(-1, -2) @ dO.abs() + u * dV.abs()
    acc = kf * (dO.abs() @ V.abs().transpose(-1, -2)) \
        + (dO * oi).abs().sum(-1, keepdim=True)
    a_dS = u * dS.abs() + scale * P * (e * (dP.abs() + delta.abs())
                                       + 2.0 ** -21 * acc)
    tol_dQ = a_dS @ K.abs() + u * dQ.abs()
    tol_dK = a_dS.transpose(-1, -2) @ Q.abs() + u * dK.abs()
    return SimpleNamespace(
        out=dict(O=O, dQ=dQ, dK=dK, dV=dV),
        tol=dict(O=tol_O, dQ=tol_dQ, dK=tol_dK, dV=tol_dV))


def ratios(got, ref):
    """Worst err / tol per output (0/0 counts as 0: an exact zero under a
    zero bound is inside it; a non-zero error under a zero bound is inf)."""
    res = {}
    for name in OUTPUTS:
        err = (got[name].double() - ref.out[name]).abs()
        tol = ref.tol[name]
        r = torch.where(err > 0, err / tol, torch.zeros_like(err))
        res[name] = float(r.max())
    return res


# ---------------------------------------------------------------- emulation
def _bf(x):
    return x.to(torch.bfloat16).float()


MUTANTS = ("drop_last_keys", "no_fwd_rescale", "keep_transposed_bwd",
           "mask_of_batch0", "ds_without_scale", "k2_stats_row_plus_16")


def emulate(q, k, v, dout, scale, add_mask=None, keep=None, p_drop=0.0,
            o_in=None, mutant=None):
    """fp32 torch model of the three kernels with bf16 casts at their
    rounding points (module header). `mutant` (one of MUTANTS) plants a
    deliberate bug; only tests/test_attention_model.py uses it, to show
    that the bound rejects it. Returns {name: bf16 tensor}."""
    assert mutant is None or mutant in MUTANTS
    scale = _f32(scale)
    scale2 = float(np.float32(scale) * np.float32(LOG2E_F32))
    rk = _rkeep(p_drop)
    Q, K, V, dO = (t.float() for t in (q, k, v, dout))
    S = q.size(-2)
    sv = (Q @ K.transpose(-1, -2)) * scale2
    if add_mask is not None:
        am = add_mask.float()
        if mutant == "mask_of_batch0":
            am = am.clone()
            am[1] = am[0]
        sv = sv + (am * LOG2E_F32)[:, None, None, :]
    if mutant == "drop_last_keys":
        sv = sv.clone()
        sv[..., S - 16:] = -1e30
    kp = keep.float() if keep is not None else None

    # forward: online softmax over 64-key tiles
    m_run = torch.full(sv.shape[:-1] + (1,), -1e30, dtype=torch.float32,
                       device=sv.device)
    l_run = torch.zeros_like(m_run)
    acc = torch.zeros_like(Q)
    for kt in range(0, S, 64):
        t = sv[..., kt:kt + 64]
        m_new = torch.maximum(m_run, t.amax(-1, keepdim=True))
        alpha = torch.exp2(m_run - m_new)
        pt = torch.exp2(t - m_new)
        l_run = l_run * alpha + pt.sum(-1, keepdim=True)
        if kp is not None:
            pt = pt * kp[..., kt:kt + 64]
        acc = acc * alpha + _bf(pt) @ V[..., kt:kt + 64, :]
        m_run = m_new
    rk_fwd = 1.0 if mutant == "no_fwd_rescale" else rk
    O = (acc / l_run * rk_fwd).to(torch.bfloat16)

    # backward K1 (per query block): delta, dS, dQ
    oi = (O if o_in is None else o_in).float()
    delta = (dO * oi).sum(-1, keepdim=True)
    kb = kp
    if kb is not None and mutant == "keep_transposed_bwd":
        kb = kb.transpose(-1, -2)
    dp = dO @ V.transpose(-1, -2)
    if kb is not None:
        dp = dp * rk * kb
    sc = 1.0 if mutant == "ds_without_scale" else scale
    p = torch.exp2(sv - m_run) / l_run
    ds = _bf(p * (dp - delta) * sc)
    dQ = (ds @ K).to(torch.bfloat16)

    # backward K2 (per key block): re-reads m, l, delta per query column
    m2, l2, d2 = m_run, l_run, delta
    if mutant == "k2_stats_row_plus_16":
        m2, l2, d2 = (torch.roll(x, -16, dims=-2) for x in (m2, l2, d2))
    p2 = torch.exp2(sv - m2) / l2
    pd = p2 if kb is None else p2 * rk * kb
    ds2 = _bf(p2 * (dp - d2) * sc)
    dV = (_bf(pd).transpose(-1, -2) @ dO).to(torch.bfloat16)
    dK = (ds2.transpose(-1, -2) @ Q).to(torch.bfloat16)
    return dict(O=O, dQ=dQ, dK=dK, dV=dV)


# ------------------------------------------------------------ dropout hash
def drop_keep(B, H, S, p, seed):
    """numpy uint32 replica of the kernels' drop_hash and threshold:
    keep[b, h, q, k] = hash(seed, b*H+h, q, k) >= thresh. Returns a uint8
    torch tensor [B, H, S, S] (1 = kept), like ext.attn_dropmask."""
    thresh = int(min(np.float32(p) * np.float32(4294967296.0),
                     np.float32(4294967040.0)))
    M32 = np.uint64(0xFFFFFFFF)
    seed32 = np.uint64(int(seed) & 0xFFFFFFFF)
    bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
    qi = np.arange(S, dtype=np.uint64)[None, :, None]
    ki = np.arange(S, dtype=np.uint64)[None, None, :]
    x = (seed32 ^ ((bh * np.uint64(0x9E3779B9)) & M32)
         ^ ((qi * np.uint64(0x85EBCA6B)) & M32)
         ^ ((ki * np.uint64(0xC2B2AE35)) & M32))
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    keep = (x >= np.uint64(thresh)).astype(np.uint8)
    return torch.from_numpy(keep.reshape(B, H, S, S))


# ----------------------------------------------------------- bounded cases
def fwd_rb(S):
    """Forward template the launcher picks: 128-row blocks from S = 256."""
    return 2 if S >= 256 else 1


def make_case(variant, D, S, p_drop=0.0):
    B = 3 if variant in ("mask", "mask_drop") else 2
    name = f"{variant}-D{D}-S{S}" + (f"-p{p_drop}" if p_drop else "")
    return SimpleNamespace(id=name, variant=variant, D=D, S=S, B=B, H=3,
                           p_drop=p_drop, seed=12345 + S + D)


# (D, S) shapes: S=32 one partial tile; 96 partial key tile and q-block;
# 160 three key tiles (double buffer wraps); 256 first RB=2, no partials;
# 288 RB=2 with waves 1-3 of the last q-block out of range; 352 RB=2 with
# only wave 3 out of range; D=128 at both templates.
SHAPES = [(64, 32), (64, 96), (64, 160), (64, 256), (64, 288), (64, 352),
          (128, 96), (128, 288)]
# every variant below reaches an RB=1, an RB=2 and a D=128 shape
CASES = (
    [make_case("plain", D, S) for D, S in SHAPES]
    + [make_case("drop", 64, 160, 0.1), make_case("drop", 64, 288, 0.1),
       make_case("drop", 128, 96, 0.1),
       make_case("drop", 64, 96, 0.5), make_case("drop", 64, 352, 0.5),
       make_case("drop", 128, 288, 0.5)]
    + [make_case("mask", 64, 96), make_case("mask", 64, 160),
       make_case("mask", 64, 288), make_case("mask", 128, 96),
       make_case("mask", 128, 288)]
    + [make_case("mask_drop", 64, 96, 0.1),
       make_case("mask_drop", 64, 352, 0.5),
       make_case("mask_drop", 128, 288, 0.1)]
    + [make_case("peaky", 64, 160), make_case("peaky", 64, 256),
       make_case("peaky", 128, 96)]
    + [make_case("spike", 64, 96), make_case("spike", 64, 288),
       make_case("spike", 128, 288)]
)


def padding_mask(B, S, device, value=-30000.0):
    """Additive key mask [B, S], different per batch: batch 0 LEFT-padded by
    70 (the whole first 64-key tile is masked), batch 1 right-padded by 17,
    batch 2 (if any) masked entirely (softmax is shift-invariant: the
    result is plain attention over logits that carry the mask's fp32
    rounding)."""
    assert S >= 96
    mask = torch.zeros(B, S, dtype=torch.float32, device=device)
    mask[0, :70] = value
    mask[1, S - 17:] = value
    if B > 2:
        mask[2, :] = value
    return mask


def make_inputs(case, device):
    """bf16 q, k, v, dout from a seeded generator of `device`, plus scale,
    mask, p_drop and seed of the case."""
    g = torch.Generator(device=device)
    g.manual_seed(1000 + case.S + case.D)
    shape = (case.B, case.H, case.S, case.D)

    def rnd(mul=1.0):
        x = torch.randn(shape, generator=g, device=device,
                        dtype=torch.float32)
        return (x * mul).to(torch.bfloat16)

    mul = 3.0 if case.variant == "peaky" else 1.0
    q, k, v, dout = rnd(mul), rnd(mul), rnd(), rnd()
    if case.variant == "spike":
        # a LATE key aligned with one query: the running max jumps at the
        # last tile for most rows, so the online rescale fires there
        k[..., case.S - 8, :] = (4.0 * q[..., 5, :].float()).to(
            torch.bfloat16)
    mask = None
    if case.variant in ("mask", "mask_drop"):
        mask = padding_mask(case.B, case.S, device)
    return SimpleNamespace(q=q, k=k, v=v, dout=dout,
                           scale=1.0 / math.sqrt(case.D), add_mask=mask,
                           p_drop=case.p_drop, seed=case.seed)


# ------------------------------------------------------------ exact inputs
SELECT_SHAPES = [(64, 96), (64, 288), (128, 160)]
SELECT_SCALE = 0.125


def selection_inputs(B, H, S, D, device):
    """Exact-selection family. k_j is the +-1 code of j (9 bits, repeated
    D // 9 times, rest 0) and q_i = 64 * k_pi(i), pi a permutation that is
    offset differently per (b, h). With scale = 0.125 the logit of the
    selected key is 8 * 9 * (D // 9) and every other key is at least
    8 * 2 * (D // 9) below it: >= 112 in natural units, >= 161 in the log2
    domain, so every other probability underflows to exactly 0 in fp32,
    l = 1, and O[i] = V[pi(i)], dV[pi(i)] = dO[i], dQ = dK = 0 bit for bit
    (V, dO small integers: every product and sum is exact).
    Returns q, k, v, dout (bf16) and pi [B, H, S] (long)."""
    assert S <= 512
    g = torch.Generator(device=device)
    g.manual_seed(77 + S + D)
    j = torch.arange(S, device=device)
    bits = ((j[:, None] >> torch.arange(9, device=device)) & 1) * 2 - 1
    code = torch.zeros(S, D, device=device)
    code[:, :9 * (D // 9)] = bits.float().repeat(1, D // 9)
    bh = torch.arange(B * H, device=device).view(B, H, 1)
    pi = (37 * j.view(1, 1, S) + 11 + 13 * bh) % S
    assert all(len(set(row.tolist())) == S for row in pi.view(-1, S))
    k = code.expand(B, H, S, D).contiguous().to(torch.bfloat16)
    q = (64.0 * code[pi]).to(torch.bfloat16)
    v = torch.randint(-4, 5, (B, H, S, D), generator=g, device=device
                      ).to(torch.bfloat16)
    dout = torch.randint(-4, 5, (B, H, S, D), generator=g, device=device
                         ).to(torch.bfloat16)
    return q, k, v, dout, pi


def selection_expected(v, dout, pi, keep=None):
    """O and dV the selection family must give exactly (rk = 2 under
    p = 0.5 dropout; keep is the kernels' keep-mask or None)."""
    D = v.size(-1)
    idx = pi[..., None].expand(-1, -1, -1, D)
    O = torch.gather(v.float(), 2, idx)
    dsel = dout.float()
    if keep is not None:
        f = 2.0 * torch.gather(keep.float(), 3, pi[..., None])
        O = O * f
        dsel = dsel * f
    dV = torch.zeros_like(O).scatter_(2, idx, dsel)
    return O.to(torch.bfloat16), dV.to(torch.bfloat16)


# (S, live key ranges per batch or None): power-of-two live counts
UNIFORM_SHAPES = [(96, ((32, 96), (64, 96))), (256, None)]


def uniform_inputs(B, H, S, D, live, device):
    """Exact-uniform family: Q = 0 makes every live logit 0, so P = 1/n on
    the n live keys (n a power of two: exact) and 0 elsewhere. V, dO small
    integers: O = mean of V over live keys and dV = (1/n) sum_q dO are
    exact in fp32, and what is stored is their correctly rounded bf16.
    dK = dS^T Q = 0 exactly. Returns q, k, v, dout, add_mask, live[B, S]."""
    g = torch.Generator(device=device)
    g.manual_seed(55 + S)
    q = torch.zeros(B, H, S, D, device=device, dtype=torch.bfloat16)
    k = torch.randn(B, H, S, D, generator=g, device=device
                    ).to(torch.bfloat16)
    v = torch.randint(-4, 5, (B, H, S, D), generator=g, device=device
                      ).to(torch.bfloat16)
    dout = torch.randint(-2, 3, (B, H, S, D), generator=g, device=device
                         ).to(torch.bfloat16)
    alive = torch.ones(B, S, dtype=torch.bool, device=device)
    mask = None
    if live is not None:
        alive[:] = False
        for b, (lo, hi) in enumerate(live):
            alive[b, lo:hi] = True
        mask = torch.zeros(B, S, dtype=torch.float32, device=device)
        mask.masked_fill_(~alive, -30000.0)
    return q, k, v, dout, mask, alive


def uniform_expected(v, dout, alive):
    """bf16 O, dV of the uniform family: the exact fp32 values, rounded."""
    B, H, S, D = v.shape
    w = alive.double()[:, None, :, None]              # [B,1,S,1]
    n = w.sum(2, keepdim=True)
    O = ((v.double() * w).sum(2, keepdim=True) / n).expand(B, H, S, D)
    dV = dout.double().sum(2, keepdim=True) / n * w
    return O.to(torch.bfloat16), dV.to(torch.bfloat16)
