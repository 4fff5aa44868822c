"""Fused optimizer kernels under every flag, vs torch.optim in float64.

The flag table of tests/test_optimizer_matrix.py, for the five classes with
a fused HIP kernel, through apply_flat (what the engine calls per bucket)
and through the kernels directly. Three steps on float64 copies of the same
fp32 parameter and gradients are the reference.

Bound (elementwise fp32 rule): |p - p_ref| <= 2^-20 * (|p| + sum over steps
of U_t), U_t the sum of |terms| of that step's update, built from the
reference's own state in float64 (_update_terms). 2^-20 is 16 fp32 ulps:
each step rounds the gradient term, the state updates, sqrt, the division
and the final subtraction once each, and the fp32 hyper-parameters (lr,
1 - beta, lr / bc1) carry one rounding each.

Sizes: scalar tail only (1, 3), exactly one float4 (4), float4 + tail (5,
1023) and 1024 * 256 * 4 + 3 (more than one block per CU, with a tail).
"""
import math

import pytest
import torch

from autodist_amd.parallel import apply as apply_mod
from tests.test_optimizer_matrix import CASES, make_grads

pytestmark = pytest.mark.gpu

FUSED = ("SGD", "Adam", "AdamW", "Adagrad", "RMSprop")
SIZES = [1, 3, 4, 5, 1023, 1024 * 256 * 4 + 3]
FUSED_CASES = [(c, i) for c in FUSED for i in range(len(CASES[c]))]
U20 = 2.0 ** -20


@pytest.fixture(scope="module")
def ext():
    from autodist_amd.ops import api
    assert api.has_gpu_ops(), "HIP extension must be built on a GPU box"
    return api.ext()


def _get(state, key, like):
    return state[key].double() if key in state else torch.zeros_like(like)


def _update_terms(cls_name, hyper, p_prev, g, st_prev, st_new, step):
    """Sum of |terms| of one update (U) and of the gradient term (gp), in
    float64 from the reference's state before / after the step."""
    lr, wd = hyper["lr"], hyper.get("weight_decay", 0.0)
    decoupled = cls_name == "AdamW" or hyper.get("decoupled_weight_decay",
                                                 False)
    gp = g.abs() if decoupled else g.abs() + wd * p_prev.abs()
    if cls_name == "SGD":
        mu = hyper["momentum"]
        d = gp
        if mu:
            b = gp if step == 1 else (
                mu * _get(st_prev, "momentum_buffer", g).abs()
                + abs(1 - hyper["dampening"]) * gp)
            d = gp + mu * b if hyper["nesterov"] else b
        return lr * d, gp, None
    if cls_name in ("Adam", "AdamW"):
        b1, b2 = hyper["betas"]
        m_abs = b1 * _get(st_prev, "exp_avg", g).abs() + (1 - b1) * gp
        v = st_new["max_exp_avg_sq" if hyper["amsgrad"] else "exp_avg_sq"]
        denom = v.double().sqrt() / math.sqrt(1 - b2 ** step) + hyper["eps"]
        u = lr / (1 - b1 ** step) * m_abs / denom
        if decoupled:
            u = u + lr * wd * p_prev.abs()
        return u, gp, None
    if cls_name == "Adagrad":
        clr = lr / (1 + (step - 1) * hyper["lr_decay"])
        return clr * gp / (st_new["sum"].double().sqrt() + hyper["eps"]), \
            gp, None
    assert cls_name == "RMSprop"
    sq = st_new["square_avg"].double()
    if hyper["centered"]:
        sq = sq - st_new["grad_avg"].double() ** 2
    ratio = gp / (sq.sqrt() + hyper["eps"])
    if hyper["momentum"] > 0:
        return lr * (hyper["momentum"]
                     * _get(st_prev, "momentum_buffer", g).abs() + ratio), \
            gp, ratio
    return lr * ratio, gp, ratio


_FIRST_MOMENTS = ("momentum_buffer", "exp_avg", "grad_avg")
_SECOND_MOMENTS = ("exp_avg_sq", "max_exp_avg_sq", "sum", "square_avg")


def _check(where, got, ref, tol):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol)
    assert not bad.any(), (
        f"{where}: {int(bad.sum())} of {bad.numel()} outside the bound, "
        f"max err/tol {(err / tol).max().item():.3f}, "
        f"max err {err.max().item():.3e}")


def _run(cls_name, kw, n, steps, step_fn, seed=0):
    p0, grads = make_grads(n, steps, seed=seed, device="cuda")
    p_ref = torch.nn.Parameter(p0.double())
    opt = getattr(torch.optim, cls_name)([p_ref], **kw)
    hyper = {k: v for k, v in opt.param_groups[0].items() if k != "params"}
    p = p0.clone()
    state = apply_mod.make_state(cls_name, p, hyper)
    u_sum = torch.zeros_like(p_ref.data)
    g_sum, g2_sum, r_sum = (torch.zeros_like(u_sum) for _ in range(3))
    p_max = p_ref.detach().abs().clone()
    for step, g in enumerate(grads, 1):
        gd = -g.double() if hyper["maximize"] else g.double()
        p_prev = p_ref.detach().clone()
        st_prev = {k: v.clone() for k, v in opt.state[p_ref].items()}
        p_ref.grad = g.double()
        opt.step()
        st_new = opt.state[p_ref]
        u, gp, ratio = _update_terms(cls_name, hyper, p_prev, gd, st_prev,
                                     st_new, step)
        u_sum += u
        g_sum += gp
        g2_sum += gp * gp
        r_sum += ratio if ratio is not None else 0.0
        p_max = torch.maximum(p_max, p_ref.detach().abs())
        step_fn(cls_name, p, g.clone(), state, hyper)
        where = f"{cls_name} {kw} n={n} step {step}"
        for key in st_new:
            # RMSprop's step is a counter torch's update never reads
            assert key in state or (cls_name, key) == ("RMSprop", "step"), \
                f"{where}: state {key!r} missing"
        _check(where + " param", p, p_ref.detach(), U20 * (p_max + u_sum))
        for key, ref in st_new.items():
            if key not in state:
                continue
            if key == "step":
                assert float(state[key]) == float(ref)
            elif key in _FIRST_MOMENTS:
                acc = r_sum if (cls_name, key) == (
                    "RMSprop", "momentum_buffer") else g_sum
                _check(f"{where} {key}", state[key], ref.double(),
                       U20 * (ref.double().abs() + acc))
            else:
                assert key in _SECOND_MOMENTS, key
                _check(f"{where} {key}", state[key], ref.double(),
                       U20 * (ref.double().abs() + g2_sum))
    return state


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("case", FUSED_CASES,
                         ids=[f"{c}-{i}" for c, i in FUSED_CASES])
def test_apply_flat_matches_torch_optim(ext, case, n):
    cls_name, idx = case
    kw = CASES[cls_name][idx]
    state = _run(cls_name, kw, n, 3, apply_mod.apply_flat, seed=idx)
    if kw.get("amsgrad"):
        # no amsgrad kernel: routed to the torch path, which keeps the max
        assert "max_exp_avg_sq" in state


def _direct_step(ext):
    """The kernels called with explicit arguments, not through
    ops.api.fused_apply."""
    def step_fn(cls_name, p, g, state, h):
        mx = bool(h["maximize"])
        if cls_name == "SGD":
            first = "momentum_buffer" not in state
            if first:
                state["momentum_buffer"] = torch.empty_like(p)
            ext.fused_sgd(p, g, state["momentum_buffer"], h["lr"],
                          h["momentum"], h["dampening"], h["weight_decay"],
                          h["nesterov"], first, mx)
        elif cls_name in ("Adam", "AdamW"):
            state["step"] += 1
            t = float(state["step"])
            b1, b2 = h["betas"]
            ext.fused_adam(p, g, state["exp_avg"], state["exp_avg_sq"],
                           h["lr"], b1, b2, h["eps"], h["weight_decay"],
                           cls_name == "AdamW", 1 - b1 ** t,
                           math.sqrt(1 - b2 ** t), mx)
        elif cls_name == "Adagrad":
            state["step"] += 1
            clr = h["lr"] / (1 + (float(state["step"]) - 1) * h["lr_decay"])
            ext.fused_adagrad(p, g, state["sum"], clr, h["eps"],
                              h["weight_decay"], mx)
        else:
            ext.fused_rmsprop(p, g, state["square_avg"],
                              state.get("grad_avg"),
                              state.get("momentum_buffer"), h["lr"],
                              h["alpha"], h["eps"], h["weight_decay"],
                              h["momentum"], mx)
    return step_fn


@pytest.mark.parametrize("cls_name,kw", [
    ("SGD", dict(lr=0.05, momentum=0.9, dampening=0.3, maximize=True)),
    ("SGD", dict(lr=0.05, momentum=0.9, dampening=0.3, weight_decay=0.01,
                 nesterov=False, maximize=True)),
    ("Adam", dict(lr=1e-2, weight_decay=0.02, maximize=True)),
    ("AdamW", dict(lr=1e-2, weight_decay=0.02, maximize=True)),
    ("Adagrad", dict(lr=0.1, weight_decay=0.01, maximize=True)),
    ("RMSprop", dict(lr=0.01, momentum=0.5, centered=True, maximize=True)),
], ids=lambda v: v if isinstance(v, str) else "")
def test_kernels_direct_maximize_dampening(ext, cls_name, kw):
    for n in (5, 1023):
        _run(cls_name, kw, n, 3, _direct_step(ext), seed=9)
