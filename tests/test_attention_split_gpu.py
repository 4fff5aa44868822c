"""Split-KV attention forward (csrc/attention_split.hip): partial-softmax
kernel + combine, through ext.attn_fwd_split and fused_sdpa(kv_splits=...).

Reference, per-element bound tol, margin K_MARGIN and inputs come from
tests/attention_ref.py. Its error model applies unchanged: P is still staged
bf16 against a running maximum; the combine adds a few fp32 roundings, which
the margin covers. Shapes: T = ceil(S / 64) key tiles, B*H = 6 or 9.
"""
import functools

import pytest
import torch

from tests import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"

# D, S, splits: S96 two tiles, the second partial (RB=1); S160 uneven 2 + 1;
# S288 RB=2, five tiles, last split one partial tile, 5 = a tile per split;
# D=128 at both RB; 7 > T clamps to 2
BOUNDED = [(64, 96, 2), (64, 160, 2), (64, 288, 2), (64, 288, 3),
           (64, 288, 5), (128, 96, 2), (128, 288, 3), (64, 96, 7)]
EXACT = [(64, 96, 2), (64, 288, 3), (128, 96, 2)]


@pytest.fixture(scope="module")
def ext():
    from autodist_amd.ops import api
    assert api.has_gpu_ops(), "HIP extension must be built on a GPU box"
    return api.ext()


@functools.lru_cache(maxsize=None)
def _case(variant, D, S):
    """Inputs and float64 forward reference, computed once per shape."""
    x = ar.make_inputs(ar.make_case(variant, D, S), DEV)
    return x, ar.reference(x.q, x.k, x.v, x.dout, x.scale, x.add_mask)


def _within(label, got, ref, names=("O",)):
    for n in names:
        assert torch.isfinite(got[n].float()).all(), n
        err = (got[n].double() - ref.out[n]).abs()
        tol = ar.K_MARGIN * ref.tol[n]
        worst = float(torch.where(err > 0, err / tol, err).max())
        print("RATIO", label, f"{n}={worst:.3f}")   # err / (k * tol)
        assert (err <= tol).all(), f"{label} {n}: err/(k tol) {worst:.3f}"


@pytest.mark.parametrize("variant", ["plain", "mask", "peaky", "spike"])
@pytest.mark.parametrize("D,S,splits", BOUNDED)
def test_bounded(ext, variant, D, S, splits):
    x, ref = _case(variant, D, S)
    o = ext.attn_fwd_split(x.q, x.k, x.v, x.scale, x.add_mask, splits)
    _within(f"{variant}-D{D}-S{S}-n{splits}", dict(O=o), ref)
    if splits > (S + 63) // 64:
        assert torch.equal(o, ext.attn_fwd_split(
            x.q, x.k, x.v, x.scale, x.add_mask, (S + 63) // 64))


@pytest.mark.parametrize("variant", ["plain", "mask"])
@pytest.mark.parametrize("D,S", [(64, 96), (64, 288), (128, 96)])
def test_one_split_bit_equal_to_attn_fwd(ext, variant, D, S):
    x, _ = _case(variant, D, S)
    assert torch.equal(
        ext.attn_fwd_split(x.q, x.k, x.v, x.scale, x.add_mask, 1),
        ext.attn_fwd(x.q, x.k, x.v, x.scale, x.add_mask))


@pytest.mark.parametrize("D,S,splits", EXACT)
def test_bit_exact_families(ext, D, S, splits):
    """A -inf mask equals the -30000 mask (batch 0 masks the whole first
    tile: split 0 of S96 has no live key and must get weight 0); transposed
    views of a qkv projection equal the contiguous call; two calls agree."""
    x, _ = _case("plain", D, S)
    B, H = x.q.shape[:2]
    m_fin = ar.padding_mask(B, S, DEV)
    m_inf = ar.padding_mask(B, S, DEV, value=float("-inf"))
    fin = ext.attn_fwd_split(x.q, x.k, x.v, x.scale, m_fin, splits)
    inf = ext.attn_fwd_split(x.q, x.k, x.v, x.scale, m_inf, splits)
    assert torch.isfinite(inf.float()).all() and torch.equal(inf, fin)
    qkv = torch.stack([x.q, x.k, x.v]).permute(1, 3, 0, 2, 4).contiguous()
    qv, kv, vv = (qkv[:, :, i].transpose(1, 2) for i in range(3))  # [B,H,S,D]
    assert not qv.is_contiguous() and torch.equal(kv, x.k)
    assert torch.equal(
        ext.attn_fwd_split(qv, kv, vv, x.scale, m_fin, splits), fin)
    assert torch.equal(
        ext.attn_fwd_split(x.q, x.k, x.v, x.scale, m_fin, splits), fin)


def test_exact_selection(ext):
    """O[i] == V[pi(i)]: splits without the winning key get weight 0."""
    q, k, v, dout, pi = ar.selection_inputs(2, 3, 288, 64, DEV)
    o = ext.attn_fwd_split(q, k, v, ar.SELECT_SCALE, None, 3)
    assert torch.equal(o, ar.selection_expected(v, dout, pi)[0])


@pytest.mark.parametrize("variant", ["plain", "mask"])
def test_fused_sdpa_kv_splits_with_backward(variant):
    from autodist_amd.ops.fused_attention import fused_sdpa
    x, _ = _case(variant, 64, 160)
    res = {}
    for n in (2, 1):
        q, k, v = (t.clone().requires_grad_(True) for t in (x.q, x.k, x.v))
        o = fused_sdpa(q, k, v, x.add_mask, kv_splits=n)
        o.backward(x.dout)
        res[n] = dict(O=o.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)
        ref = ar.reference(x.q, x.k, x.v, x.dout, x.scale, x.add_mask,
                           o_in=res[n]["O"])
        _within(f"sdpa-{variant}-n{n}", res[n], ref, names=ar.OUTPUTS)
    if torch.equal(res[1]["O"], res[2]["O"]):   # same o in: same backward
        for name in ("dQ", "dK", "dV"):
            assert torch.equal(res[1][name], res[2][name]), name


def test_refusals(ext):
    from autodist_amd.ops.fused_attention import fused_sdpa
    x, _ = _case("plain", 64, 96)
    with pytest.raises(ValueError):
        fused_sdpa(x.q, x.k, x.v, dropout_p=0.1, kv_splits=2)
    with pytest.raises(ValueError):
        fused_sdpa(x.q, x.k, x.v, kv_splits=0)
    with pytest.raises(RuntimeError):
        ext.attn_fwd_split(x.q, x.k, x.v, x.scale, None, 0)
    with pytest.raises(RuntimeError):
        ext.attn_fwd_split(x.q, x.k, x.v, x.scale, None, 2, 0.1)
    q = torch.randn(2, 3, 96, 96, device=DEV).to(torch.bfloat16)
    assert torch.equal(
        fused_sdpa(q, q, q, kv_splits=2),
        torch.nn.functional.scaled_dot_product_attention(q, q, q))


@pytest.mark.parametrize("env,called", [("1", "attn_fwd"),
                                        ("3", "attn_fwd_split")])
def test_env_override(ext, monkeypatch, env, called):
    """B1 H2 S512 is a shape the dispatch rule may split; the variable
    decides for kv_splits=None."""
    from autodist_amd.ops import api, fused_attention
    calls = []

    class Recorder:
        def __getattr__(self, name):
            calls.append(name)
            return getattr(ext, name)

    monkeypatch.setattr(api, "ext", Recorder)
    monkeypatch.setenv("AUTODIST_ATTN_KV_SPLITS", env)
    q = torch.randn(1, 2, 512, 64, device=DEV).to(torch.bfloat16)
    with torch.no_grad():
        fused_attention.fused_sdpa(q, q, q)
    assert calls == [called]
