"""MFMA attention forward + both backward kernels across their geometries.

The kernels (csrc/attention.hip, csrc/attention_bwd.hip) are called directly
through ext.attn_fwd / ext.attn_bwd and compared with the float64 reference
of tests/attention_ref.py, whose header derives the per-element bound tol
and whose CPU companion tests/test_attention_model.py measures the one
margin k (K_MARGIN) and shows that planted bugs leave k * tol. The backward
reference takes the kernel's own bf16 O, which is an input of attn_bwd.

  (a) bounded cases: |kernel - ref| <= k * tol per element of O, dQ, dK, dV
      over the shapes of attention_ref.SHAPES (partial key tiles and
      q-blocks, 3+ key tiles so the forward's double buffer wraps, RB=2 with
      whole waves out of range, both head dims) crossed with dropout, a
      per-batch key mask, both together, peaky softmax and a late spiked
      key; B*H = 6 or 9 is no multiple of 8, so the bh = block % NBH
      swizzle and the mask's bh / H indexing matter. Mixed-stride q/k/v
      views are bit-equal to the contiguous call.
  (b) a -inf mask gives finite results bit-equal to the -30000 mask.
  (c) exact selection and (d) exact uniform attention: integer-valued
      inputs for which every index map (tiles, RB, both LDS transposes, the
      hash's (bh, q, k) arguments in all three kernels) is pinned with
      torch.equal and no tolerance.
  (e) ext.attn_dropmask equals the independent numpy replica of the hash.
"""
import pytest
import torch

from tests import attention_ref as ar

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def ext():
    from autodist_amd.ops import api
    assert api.has_gpu_ops(), "HIP extension must be built on a GPU box"
    return api.ext()


def _fwd_bwd(ext, q, k, v, dout, scale, mask=None, p_drop=0.0, seed=0):
    o = ext.attn_fwd(q, k, v, scale, mask, p_drop, seed)
    dq, dk, dv = ext.attn_bwd(q, k, v, o, dout, scale, mask, p_drop, seed)
    return dict(O=o, dQ=dq, dK=dk, dV=dv)


def _within(label, got, ref, names=ar.OUTPUTS):
    r = ar.ratios(got, ref)
    # err / (k * tol) per output: the figures of docs/KERNELS.md
    print("RATIO", label, " ".join(
        f"{n}={r[n] / ar.K_MARGIN:.3f}" for n in names))
    for name in names:
        assert torch.isfinite(got[name].float()).all(), name
        err = (got[name].double() - ref.out[name]).abs()
        tol = ar.K_MARGIN * ref.tol[name]
        bad = ~(err <= tol)
        assert not bad.any(), (
            f"{label} {name}: {int(bad.sum())} of {bad.numel()} outside the "
            f"bound, max err/tol {r[name] / ar.K_MARGIN:.3f} (k = "
            f"{ar.K_MARGIN}), max err {err.max().item():.3e}")


# ------------------------------------------------------------ (a) bounded
@pytest.mark.parametrize("case", ar.CASES, ids=lambda c: c.id)
def test_bounded(ext, case):
    x = ar.make_inputs(case, DEV)
    keep = None
    if case.p_drop:
        keep = ext.attn_dropmask(case.B, case.H, case.S, case.p_drop,
                                 case.seed, x.q.device)
    got = _fwd_bwd(ext, x.q, x.k, x.v, x.dout, x.scale, x.add_mask,
                   x.p_drop, x.seed)
    ref = ar.reference(x.q, x.k, x.v, x.dout, x.scale, x.add_mask, keep,
                       x.p_drop, o_in=got["O"])
    _within(case.id, got, ref)


@pytest.mark.parametrize("D,S", [(64, 96), (64, 288), (128, 96)])
def test_mixed_strides_bit_equal(ext, D, S):
    """q a view of a [B,S,3,H,D] projection, k contiguous, v the first half
    of a [B,H,S,2D] tensor: three different (sb, sh, ss) triples, so a
    kernel that used one tensor's stride for another reads other data."""
    case = ar.make_case("mask_drop", D, S, 0.1)
    x = ar.make_inputs(case, DEV)
    B, H = case.B, case.H
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    qkv = torch.randn(B, S, 3, H, D, generator=g, device=DEV
                      ).to(torch.bfloat16)
    qkv[:, :, 0] = x.q.transpose(1, 2)
    q_view = qkv[:, :, 0].transpose(1, 2)
    vv = torch.randn(B, H, S, 2 * D, generator=g, device=DEV
                     ).to(torch.bfloat16)
    vv[..., :D] = x.v
    v_view = vv[..., :D]
    assert torch.equal(q_view, x.q) and torch.equal(v_view, x.v)
    strides = {q_view.stride()[:3], x.k.stride()[:3], v_view.stride()[:3]}
    assert len(strides) == 3 and q_view.stride(3) == v_view.stride(3) == 1
    base = _fwd_bwd(ext, x.q, x.k, x.v, x.dout, x.scale, x.add_mask,
                    x.p_drop, x.seed)
    got = _fwd_bwd(ext, q_view, x.k, v_view, x.dout, x.scale, x.add_mask,
                   x.p_drop, x.seed)
    for name in ar.OUTPUTS:
        assert torch.equal(got[name], base[name]), name


# ----------------------------------------------------------- (b) -inf mask
@pytest.mark.parametrize("D,S", [(64, 96), (64, 288), (128, 96)])
def test_neg_inf_mask_equals_finite_mask(ext, D, S):
    """-inf on the same keys as -30000 (the whole first key tile of batch 0
    included; every row keeps live keys): the probabilities are exactly 0
    either way, so all four outputs are finite and bit-equal."""
    x = ar.make_inputs(ar.make_case("plain", D, S), DEV)
    m_fin = ar.padding_mask(2, S, DEV)
    m_inf = ar.padding_mask(2, S, DEV, value=float("-inf"))
    assert torch.equal(m_fin != 0, torch.isinf(m_inf))
    fin = _fwd_bwd(ext, x.q, x.k, x.v, x.dout, x.scale, m_fin)
    inf = _fwd_bwd(ext, x.q, x.k, x.v, x.dout, x.scale, m_inf)
    for name in ar.OUTPUTS:
        assert torch.isfinite(inf[name].float()).all(), name
        assert torch.equal(inf[name], fin[name]), name
    # masked keys receive no gradient at all
    dead = (m_fin != 0)[:, None, :, None].expand_as(x.q)
    assert not inf["dK"][dead].any() and not inf["dV"][dead].any()


# ------------------------------------------------------ (c) exact selection
@pytest.mark.parametrize("D,S", ar.SELECT_SHAPES)
@pytest.mark.parametrize("p_drop", [0.0, 0.5])
def test_exact_selection(ext, D, S, p_drop):
    B, H, seed = 2, 3, 4242
    q, k, v, dout, pi = ar.selection_inputs(B, H, S, D, DEV)
    keep = None
    if p_drop:      # the independent replica, not the kernels' own hash
        keep = ar.drop_keep(B, H, S, p_drop, seed).to(DEV)
    got = _fwd_bwd(ext, q, k, v, dout, ar.SELECT_SCALE, None, p_drop, seed)
    O, dV = ar.selection_expected(v, dout, pi, keep)
    assert torch.equal(got["O"], O)
    assert torch.equal(got["dV"], dV)
    assert torch.equal(got["dQ"], torch.zeros_like(q))
    assert torch.equal(got["dK"], torch.zeros_like(q))


# -------------------------------------------------------- (d) exact uniform
@pytest.mark.parametrize("D,S,live", [
    (64,) + ar.UNIFORM_SHAPES[0], (64,) + ar.UNIFORM_SHAPES[1],
    (128,) + ar.UNIFORM_SHAPES[0]])
def test_exact_uniform(ext, D, S, live):
    B, H = 2, 3
    q, k, v, dout, mask, alive = ar.uniform_inputs(B, H, S, D, live, DEV)
    got = _fwd_bwd(ext, q, k, v, dout, 0.125, mask)
    O, dV = ar.uniform_expected(v, dout, alive)
    assert torch.equal(got["O"], O)
    assert torch.equal(got["dV"], dV)
    assert torch.equal(got["dK"], torch.zeros_like(q))
    ref = ar.reference(q, k, v, dout, 0.125, mask, o_in=got["O"])
    _within(f"uniform-D{D}-S{S}", got, ref, names=("dQ",))


# --------------------------------------------------------- (e) hash replica
@pytest.mark.parametrize("seed", [0, 12345, 2 ** 31 + 7, 2 ** 32 + 5])
def test_dropmask_matches_replica(ext, seed):
    B, H, S = 2, 3, 96
    for p in (0.1, 0.5, 0.999):
        got = ext.attn_dropmask(B, H, S, p, seed, torch.device(DEV))
        want = ar.drop_keep(B, H, S, p, seed)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(got.cpu(), want), (seed, p)
