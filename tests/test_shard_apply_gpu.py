"""The bf16-gradient ("wire") optimizer kernels of the sharded dense schedule.

bf16 -> fp32 is exact and the wire kernels are the fp32 kernels' own code
instantiated for a bf16 gradient stream, so ops.api.fused_apply_wire must be
BIT-identical to ops.api.fused_apply on grad.float(): in the parameters and
in every state tensor, over consecutive steps (momentum first step and later
steps, Adam bias correction, Adagrad lr decay).
"""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 8, 1027, 262144 + 5]  # tail only; vector+tail; >1 block

CASES = [
    ("SGD", {"lr": 0.1}),
    ("SGD", {"lr": 0.1, "momentum": 0.9}),
    ("SGD", {"lr": 0.1, "momentum": 0.9, "nesterov": True}),
    ("SGD", {"lr": 0.1, "momentum": 0.9, "dampening": 0.3}),
    ("SGD", {"lr": 0.1, "momentum": 0.9, "weight_decay": 1e-2}),
    ("SGD", {"lr": 0.1, "weight_decay": 1e-2, "maximize": True}),
    ("Adam", {"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8,
              "weight_decay": 1e-2}),
    ("Adam", {"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8,
              "maximize": True}),
    ("AdamW", {"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8,
               "weight_decay": 1e-2}),
    ("Adagrad", {"lr": 0.1, "lr_decay": 1e-2, "eps": 1e-10}),
    ("Adagrad", {"lr": 0.1, "eps": 1e-10, "weight_decay": 1e-2}),
]
_IDS = [f"{c}-{'-'.join(k for k in h if k not in ('lr', 'betas', 'eps'))}"
        .rstrip("-") for c, h in CASES]

SENTINEL = -12288.0  # exact in bf16 as well


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)


_inputs = {}


def _data(n, dev):
    """One parameter vector and three bf16 gradients per size, made once and
    never modified (every test clones what it updates)."""
    if n not in _inputs:
        gen = torch.Generator().manual_seed(n)
        p = torch.randn(n, generator=gen)
        gs = [torch.randn(n, generator=gen).to(torch.bfloat16)
              for _ in range(3)]
        _inputs[n] = (p.to(dev), [g.to(dev) for g in gs])
    return _inputs[n]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _assert_state_bitwise(st_a, st_b, what):
    assert st_a.keys() == st_b.keys(), what
    for k in st_a:
        a, b = st_a[k], st_b[k]
        assert a.shape == b.shape, (what, k)
        assert torch.equal(_bits(a.float()), _bits(b.float())), (what, k)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cls_name,hyper", CASES, ids=_IDS)
def test_wire_apply_bitwise_equals_fp32_path(gpu, cls_name, hyper, n):
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    p0, grads = _data(n, gpu)
    p_ref, p_wire = p0.clone(), p0.clone()
    st_ref = apply_mod.make_state(cls_name, p_ref, hyper)
    st_wire = copy.deepcopy(st_ref)
    for step, g in enumerate(grads):
        assert ops_api.fused_apply(cls_name, p_ref, g.float(), st_ref, hyper)
        assert ops_api.fused_apply_wire(cls_name, p_wire, g, st_wire, hyper)
        assert torch.equal(_bits(p_ref), _bits(p_wire)), \
            f"step {step}: {(p_ref - p_wire).abs().max().item()}"
        _assert_state_bitwise(st_ref, st_wire, f"step {step}")
    assert not torch.equal(p_ref, p0)  # the update did something


@pytest.mark.parametrize("k,length", [(1, 8), (3, 1024), (5, 262144 + 8)])
@pytest.mark.parametrize("cls_name,hyper", [CASES[4], CASES[8], CASES[9]],
                         ids=["SGD", "AdamW", "Adagrad"])
def test_wire_apply_on_shard_views_leaves_guards_alone(gpu, cls_name, hyper,
                                                       k, length):
    """Shard views flat[8k : 8k+L] of larger buffers, as the engine passes
    them; the elements on both sides of the shard must not change."""
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    lo, hi = 8 * k, 8 * k + length
    total = hi + 24
    p0, grads = _data(length, gpu)

    def guarded(src, dtype=torch.float32):
        buf = torch.full((total,), SENTINEL, dtype=dtype, device=gpu)
        buf[lo:hi] = src
        return buf

    p_ref = p0.clone()
    st_ref = apply_mod.make_state(cls_name, p_ref, hyper)
    flat_p = guarded(p0)
    # state held as views of guarded buffers too
    st_bufs = {key: guarded(t) for key, t in st_ref.items() if t.dim() > 0}
    st_wire = {key: (st_bufs[key][lo:hi] if key in st_bufs else t.clone())
               for key, t in st_ref.items()}
    if cls_name == "SGD":  # created by the first call otherwise
        st_bufs["momentum_buffer"] = guarded(torch.zeros(length, device=gpu))
    for step, g in enumerate(grads):
        flat_g = guarded(g, torch.bfloat16)
        if cls_name == "SGD" and step == 1:
            # move the (contiguous) buffer the first step made into a view
            st_bufs["momentum_buffer"][lo:hi] = st_wire["momentum_buffer"]
            st_wire["momentum_buffer"] = st_bufs["momentum_buffer"][lo:hi]
        assert ops_api.fused_apply(cls_name, p_ref, g.float(), st_ref, hyper)
        assert ops_api.fused_apply_wire(cls_name, flat_p[lo:hi],
                                        flat_g[lo:hi], st_wire, hyper)
        assert torch.equal(_bits(flat_p[lo:hi]), _bits(p_ref)), step
        _assert_state_bitwise(st_ref, st_wire, f"step {step}")
        for buf in [flat_p, flat_g.float()] + list(st_bufs.values()):
            guard = torch.cat([buf[:lo], buf[hi:]])
            assert torch.equal(guard, torch.full_like(guard, SENTINEL)), step


@pytest.mark.parametrize("cls_name,hyper", [CASES[1], CASES[8], CASES[9]],
                         ids=["SGD", "AdamW", "Adagrad"])
def test_misaligned_views_are_refused_host_side(gpu, cls_name, hyper):
    """A view at element offset 1 is not 16-byte aligned: fused_apply_wire
    returns False before anything is launched or any state advances, and
    apply_flat_shard still produces the torch result."""
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    n = 1027
    p0, grads = _data(n, gpu)
    g = grads[0]
    big_p = torch.cat([p0.new_zeros(1), p0])
    big_g = torch.cat([g.new_zeros(1), g])
    for p_view, g_view in ((big_p[1:], g), (p0.clone(), big_g[1:]),
                           (p0.clone()[::2], g[::2])):
        before = p_view.clone()
        st = apply_mod.make_state(cls_name, p_view.contiguous(), hyper)
        st_before = copy.deepcopy(st)
        assert not ops_api.fused_apply_wire(cls_name, p_view, g_view, st,
                                            hyper)
        assert torch.equal(p_view, before)
        _assert_state_bitwise(st, st_before, "refused call")
    # misaligned state tensor
    if cls_name != "SGD":
        p = p0.clone()
        st = apply_mod.make_state(cls_name, p, hyper)
        key = "sum" if cls_name == "Adagrad" else "exp_avg"
        st[key] = torch.cat([st[key].new_zeros(1), st[key]])[1:]
        assert not ops_api.fused_apply_wire(cls_name, p, g, st, hyper)
        assert float(st["step"]) == 0.0 and torch.equal(p, p0)
    # the dispatcher falls through to the torch composite
    p_shard = big_p[1:]
    st = apply_mod.make_state(cls_name, p_shard, hyper)
    apply_mod.apply_flat_shard(cls_name, p_shard, g, st, hyper)
    p_t = p0.clone()
    st_t = apply_mod.make_state(cls_name, p_t, hyper)
    apply_mod._APPLY[cls_name]([p_t], [g.float()], [st_t], hyper)
    assert torch.equal(_bits(p_shard), _bits(p_t))
    assert not torch.equal(p_shard, p0)
    # the extension itself refuses misaligned pointers
    with pytest.raises(RuntimeError, match="aligned"):
        ops_api.ext().fused_adagrad_wire(big_p[1:], g, torch.zeros_like(p0),
                                         0.1, 1e-10, 0.0, False)


@pytest.mark.parametrize("cls_name,hyper", [
    ("RMSprop", {"lr": 1e-2, "alpha": 0.99, "eps": 1e-8}),
    ("Adam", {"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8,
              "amsgrad": True}),
    ("Adamax", {"lr": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8}),
], ids=["RMSprop", "amsgrad", "Adamax"])
def test_classes_without_wire_kernel_fall_through(gpu, cls_name, hyper):
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    p0, grads = _data(1027, gpu)
    p_a, p_b = p0.clone(), p0.clone()
    st_a = apply_mod.make_state(cls_name, p_a, hyper)
    st_b = copy.deepcopy(st_a)
    assert not ops_api.fused_apply_wire(cls_name, p_a, grads[0], st_a, hyper)
    assert torch.equal(p_a, p0)
    _assert_state_bitwise(st_a, st_b, "refused call")
    for g in grads:
        apply_mod.apply_flat_shard(cls_name, p_a, g, st_a, hyper)
        apply_mod.apply_dense(cls_name, [p_b], [g.float()], [st_b], hyper)
    assert torch.equal(_bits(p_a), _bits(p_b))
    _assert_state_bitwise(st_a, st_b, "fall-through")
    assert not torch.equal(p_a, p0)
