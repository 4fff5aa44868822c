"""Optimizer flag matrix: engine apply layer vs torch.optim, bit for bit.

For each of the 11 classes in apply._SUPPORTED a handful of keyword sets
that together move EVERY semantic constructor flag off its default
(`maximize=True` always among them). Four steps of apply_dense run beside
opt.step() on the CPU; the parameter and every state tensor must be
torch.equal. The table (CASES) is shared with the GPU matrix in
tests/test_optimizer_matrix_gpu.py.
"""
import inspect

import pytest
import torch

from autodist_amd.ops import api as ops_api
from autodist_amd.parallel import apply as apply_mod

# Flags that choose an implementation inside torch.optim (multi-tensor,
# fused, graph-capturable, differentiable), not the update rule.
_IMPL_FLAGS = {"params", "self", "foreach", "fused", "capturable",
               "differentiable"}

CASES = {
    "SGD": [
        dict(lr=0.1, maximize=True),
        dict(lr=0.05, momentum=0.9, dampening=0.3, weight_decay=0.01,
             maximize=True),
        dict(lr=0.05, momentum=0.8, nesterov=True, weight_decay=0.02),
        dict(lr=0.1, momentum=0.5, dampening=0.25),
    ],
    "Adam": [
        dict(lr=1e-2, maximize=True),
        dict(lr=3e-3, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05,
             maximize=True),
        dict(lr=1e-2, amsgrad=True, weight_decay=0.01, maximize=True),
        dict(lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True),
    ],
    "AdamW": [
        dict(lr=1e-2, maximize=True),
        dict(lr=3e-3, betas=(0.7, 0.9), eps=1e-5, weight_decay=0.2,
             maximize=True),
        dict(lr=1e-2, amsgrad=True),
    ],
    "Adagrad": [
        dict(lr=0.1, maximize=True),
        dict(lr=0.05, lr_decay=0.1, weight_decay=0.01,
             initial_accumulator_value=0.5, eps=1e-6, maximize=True),
        dict(lr=0.05, lr_decay=0.2, initial_accumulator_value=0.1),
    ],
    "RMSprop": [
        dict(lr=0.01, maximize=True),
        dict(lr=0.02, alpha=0.9, eps=1e-6, weight_decay=0.01, momentum=0.7,
             centered=True, maximize=True),
        dict(lr=0.01, centered=True),
        dict(lr=0.01, momentum=0.5, alpha=0.95),
    ],
    "Adamax": [
        dict(lr=2e-2, maximize=True),
        dict(lr=1e-2, betas=(0.8, 0.9), eps=1e-6, weight_decay=0.05,
             maximize=True),
    ],
    "NAdam": [
        dict(lr=2e-2, maximize=True),
        dict(lr=1e-2, betas=(0.8, 0.95), eps=1e-6, weight_decay=0.05,
             momentum_decay=1e-2, maximize=True),
        dict(lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True,
             maximize=True),
    ],
    "RAdam": [
        dict(lr=2e-2, maximize=True),
        # beta2 = 0.5 keeps rho_t <= 5: the un-rectified branch
        dict(lr=1e-2, betas=(0.8, 0.5), eps=1e-6, weight_decay=0.05,
             maximize=True),
        dict(lr=1e-2, weight_decay=0.1, decoupled_weight_decay=True),
    ],
    "Adadelta": [
        dict(lr=1.0, maximize=True),
        dict(lr=0.5, rho=0.8, eps=1e-5, weight_decay=0.05, maximize=True),
    ],
    "ASGD": [
        dict(lr=0.05, maximize=True),
        # t0 = 1: averaging (mu != 1) starts inside the 4 steps
        dict(lr=0.02, lambd=1e-2, alpha=0.5, t0=1, weight_decay=0.05,
             maximize=True),
    ],
    "Rprop": [
        dict(lr=0.05, maximize=True),
        dict(lr=0.02, etas=(0.3, 1.5), step_sizes=(1e-3, 0.03),
             maximize=True),
    ],
}

ALL_CASES = [(c, i) for c in CASES for i in range(len(CASES[c]))]


def case_id(val):
    return f"{val[0]}-{val[1]}"


def make_grads(n, steps, seed=0, device="cpu"):
    g = torch.Generator().manual_seed(seed)
    p0 = torch.randn(n, generator=g)
    grads = [torch.randn(n, generator=g) for _ in range(steps)]
    return p0.to(device), [x.to(device) for x in grads]


def test_case_table_covers_every_class_and_flag():
    assert set(CASES) == set(apply_mod._SUPPORTED)
    for cls_name, kws in CASES.items():
        sig = inspect.signature(getattr(torch.optim, cls_name).__init__)
        for name, prm in sig.parameters.items():
            if name in _IMPL_FLAGS:
                continue
            assert any(name in kw and kw[name] != prm.default for kw in kws), \
                f"{cls_name}: flag {name!r} never leaves its default"
        assert any(kw.get("maximize") for kw in kws)


# torch's RMSprop counts steps but its update never reads the count; the
# engine (make_state, engine._state_keys) keeps no such counter.
_UNUSED_COUNTERS = {("RMSprop", "step")}


def _assert_state_equal(cls_name, ours, theirs, where):
    for key, ref in theirs.items():
        if (cls_name, key) in _UNUSED_COUNTERS:
            continue
        assert key in ours, f"{where}: state {key!r} missing"
        got = ours[key]
        if not torch.is_tensor(ref):
            assert float(got) == float(ref), f"{where}: state {key!r}"
            continue
        got = got if torch.is_tensor(got) else torch.tensor(got)
        assert torch.equal(got.to(ref.dtype).reshape(ref.shape), ref), \
            f"{where}: state {key!r} max |d| " \
            f"{(got.double() - ref.double()).abs().max().item():.3e}"


@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_apply_dense_bit_matches_torch_optim(case):
    cls_name, idx = case
    kw = CASES[cls_name][idx]
    n, steps = 1001, 4
    p0, grads = make_grads(n, steps, seed=idx)
    p_ref = torch.nn.Parameter(p0.clone())
    opt = getattr(torch.optim, cls_name)([p_ref], **kw)
    hyper = {k: v for k, v in opt.param_groups[0].items() if k != "params"}
    p = p0.clone()
    state = apply_mod.make_state(cls_name, p, hyper)
    for step, g in enumerate(grads, 1):
        p_ref.grad = g.clone()
        opt.step()
        apply_mod.apply_dense(cls_name, [p], [g.clone()], [state], hyper)
        where = f"{cls_name} {kw} step {step}"
        assert torch.equal(p, p_ref.detach()), \
            f"{where}: max |dparam| " \
            f"{(p - p_ref.detach()).abs().max().item():.3e}"
        _assert_state_equal(cls_name, state, opt.state[p_ref], where)


def test_fused_supported_predicate():
    for cls_name in ("SGD", "Adam", "AdamW", "Adagrad", "RMSprop"):
        assert ops_api.fused_supported(cls_name, {})
        assert ops_api.fused_supported(cls_name, {"maximize": True})
    for cls_name in ("Adam", "AdamW"):
        assert not ops_api.fused_supported(cls_name, {"amsgrad": True})
        assert ops_api.fused_supported(cls_name, {"amsgrad": False})
    # amsgrad is no flag of the other fused classes: ignored there
    assert ops_api.fused_supported("SGD", {"amsgrad": True})
    for cls_name in ("Adamax", "NAdam", "RAdam", "Adadelta", "ASGD", "Rprop",
                     "LBFGS"):
        assert not ops_api.fused_supported(cls_name, {})
    # the predicate is pure: the hyper dict is left alone
    hyper = {"amsgrad": True, "lr": 1.0}
    ops_api.fused_supported("Adam", hyper)
    assert hyper == {"amsgrad": True, "lr": 1.0}
    # fused_apply refuses before it touches the state or looks for a GPU
    state = {"step": torch.zeros(())}
    p = torch.zeros(4)
    assert not ops_api.fused_apply("Adam", p, p, state, hyper)
    assert float(state["step"]) == 0.0
