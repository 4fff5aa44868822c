"""Fused NeuMF kernels (ops/csrc/ncf_ops.hip) against the NeuMF formulas in
float64 on the same fp32 inputs.

Rule, per output (logits, loss rows, the four table gradients, every dW / db
and the head): with e_c the max error of the torch fp32 module path against
float64 and e_k the fused path's, e_k <= 4 e_c + 8 * 2^-24 * max|ref|. Both
are fp32 and differ only in summation order; 4 is the spread between two
valid orderings, the floor covers outputs where torch happens to be exact.
"""
import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(8, (16, 8)), (16, (32, 16)), (64, (256, 128, 64)),
          (8, (64, 32, 16, 8)), (24, (48, 256, 40))]
NU, NI = 11, 7   # few rows: duplicate ids in every batch of more than one


def _fused():
    from autodist_amd.ops import fused_ncf
    return fused_ncf


def _model(mf, dims, sparse):
    from autodist_amd.models.ncf import NeuMF
    torch.manual_seed(0)
    m = NeuMF(NU, NI, mf_dim=mf, mlp_dims=dims, sparse=sparse)
    with torch.no_grad():
        for t in (m.mf_user, m.mf_item, m.mlp_user, m.mlp_item):
            t.weight.normal_(0, 0.5)
    return m.cuda()


def _inputs(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    r = lambda *a, **k: torch.rand(*a, generator=g, **k)  # noqa: E731
    users = torch.randint(0, NU, (B,), generator=g).cuda()
    items = torch.randint(0, NI, (B,), generator=g).cuda()
    labels = (torch.arange(B) % 2).float().cuda()
    weight = (r(B) * 2).cuda()
    weight[::3] = 0
    return users, items, labels, weight, (r(B) - 0.5).cuda(), \
        (r(B) + 0.5).cuda()


def _dense(g):
    """A gradient as a dense tensor; sparse rows added in index order
    (to_dense coalesces with atomics: not the same bits every run)."""
    from autodist_amd.ops.sampled_softmax import _scatter_rows
    if not g.is_sparse:
        return g
    return _scatter_rows(g.size(0), g._indices()[0], g._values())


def _run(model, inp, fused, with_logit_grad=True):
    """{name: dense tensor} of every output; `fused` picks the path."""
    users, items, labels, weight, gz, gl = inp
    for p in model.parameters():
        p.grad = None
    dt = model.head.weight.dtype
    if fused:
        z, rows = _fused().neumf_forward(
            users, items, (model.mf_user, model.mf_item, model.mlp_user,
                           model.mlp_item), model.mlp, model.head, labels,
            weight)
    else:
        z = model(users, items)
        rows = F.binary_cross_entropy_with_logits(
            z, labels.to(dt), weight=weight.to(dt), reduction="none")
    total = (rows * gl.to(dt)).sum()
    if with_logit_grad:
        total = total + (z * gz.to(dt)).sum()
    total.backward()
    out = {"logits": z.detach(), "loss_rows": rows.detach()}
    for n, p in model.named_parameters():
        out[n] = _dense(p.grad)
    return out, z


def _reference(model, inp, monkeypatch, **kw):
    """(float64 outputs, torch fp32 module-path outputs)."""
    monkeypatch.setenv("AUTODIST_NCF", "torch")
    ref, _ = _run(copy.deepcopy(model).double(), inp, False, **kw)
    t32, z = _run(model, inp, False, **kw)
    assert "NeuMF" not in type(z.grad_fn).__name__
    monkeypatch.delenv("AUTODIST_NCF")
    return ref, t32


def _check(got, t32, ref, names=None):
    bad = []
    for n in names or ref:
        e_k = (got[n].double() - ref[n]).abs().max().item()
        e_c = (t32[n].double() - ref[n]).abs().max().item()
        bound = 4 * e_c + 8 * 2.0 ** -24 * ref[n].abs().max().item()
        print(f"{n}: e_k {e_k:.3e} e_c {e_c:.3e} ratio "
              f"{e_k / e_c if e_c else float('inf'):.2f} bound {bound:.3e}")
        if not e_k <= bound:
            bad.append((n, e_k, e_c, bound))
    assert not bad, bad


@pytest.mark.parametrize("sparse", [True, False])
@pytest.mark.parametrize("mf,dims", SHAPES)
@pytest.mark.parametrize("tiles,extra", [(0, 1), (1, 1), (2, 3)])
def test_numerics(tiles, extra, mf, dims, sparse, monkeypatch):
    from autodist_amd.ops import api as ops_api
    B = tiles * ops_api.ext().NEUMF_TILE + extra
    model, inp = _model(mf, dims, sparse), _inputs(B)
    users, items = inp[:2]
    if B > 1:
        assert users.unique().numel() < B and items.unique().numel() < B
    ref, t32 = _reference(model, inp, monkeypatch)
    got, z = _run(model, inp, True)
    assert type(z.grad_fn).__name__ == "_NeuMFFnBackward"
    _check(got, t32, ref)
    sparse_grads = {n: p.grad for n, p in model.named_parameters()
                    if p.grad.is_sparse}
    again, _ = _run(model, inp, True)
    assert all(torch.equal(got[n], again[n]) for n in got)
    assert bool(sparse_grads) == sparse
    if sparse:
        twin = copy.deepcopy(model)
        for t in (twin.mf_user, twin.mf_item, twin.mlp_user, twin.mlp_item):
            t.sparse = False
        dense, _ = _run(twin, inp, True)
        for n, g in sparse_grads.items():
            ids = users if "user" in n else items
            assert g.is_coalesced() == (B == 1)  # torch: nnz < 2
            assert torch.equal(g._indices()[0], ids)
            assert torch.equal(_dense(g), dense[n])


def test_bce_stability(monkeypatch):
    """|z| up to ~80 with both labels: finite loss rows within the rule, and
    no gradient at all from a row whose weight is 0."""
    model, inp = _model(8, (16, 8), True), _inputs(67)
    with torch.no_grad():
        zmax = model(inp[0], inp[1]).abs().max()
        model.head.weight.mul_(80 / zmax)
        model.head.bias.mul_(80 / zmax)
    ref, t32 = _reference(model, inp, monkeypatch, with_logit_grad=False)
    assert ref["logits"].abs().max() > 60
    for y in (0, 1):
        assert ref["logits"][inp[2] == y].abs().max() > 40
    got, _ = _run(model, inp, True, with_logit_grad=False)
    assert torch.isfinite(got["loss_rows"]).all()
    _check(got, t32, ref, ["logits", "loss_rows"])
    dead = inp[3] == 0
    for t in (model.mf_user, model.mf_item, model.mlp_user, model.mlp_item):
        assert (t.weight.grad._values()[dead] == 0).all()
        assert (t.weight.grad._values()[~dead] != 0).any()


def test_public_path(monkeypatch):
    """NeuMF.loss + backward takes the kernels; the parameters' gradients
    follow the rule against the AUTODIST_NCF=torch run of the same model."""
    model, inp = _model(64, (256, 128, 64), True), _inputs(67)
    users, items, labels = inp[:3]

    def grads(m):
        for p in m.parameters():
            p.grad = None
        loss = m.loss(users, items, labels)
        loss.backward()
        return loss, {n: _dense(p.grad) for n, p in m.named_parameters()}

    monkeypatch.setenv("AUTODIST_NCF", "torch")
    _, ref = grads(copy.deepcopy(model).double())
    _, t32 = grads(model)
    monkeypatch.delenv("AUTODIST_NCF")
    loss, got = grads(model)
    fn = loss.grad_fn.next_functions[0][0]
    assert type(fn).__name__ == "_NeuMFFnBackward"
    assert model.mf_user.weight.grad.is_sparse
    _check(got, t32, ref)


def test_refusals():
    from autodist_amd.models.ncf import NeuMF
    from autodist_amd.ops import api as ops_api
    can = _fused().can_use_fused_neumf
    ext = ops_api.ext()
    users = torch.zeros(4, dtype=torch.int64, device="cuda")
    good = NeuMF(NU, NI, 8, (16, 8)).cuda()
    assert can(good, users)
    assert not can(NeuMF(NU, NI, 12, (16, 8)).cuda(), users)
    assert not can(NeuMF(NU, NI, 8, (16, 12, 8)).cuda(), users)
    deep = (16,) * (ext.NEUMF_MAX_LAYERS + 2)
    assert not can(NeuMF(NU, NI, 8, deep).cuda(), users)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        assert not can(good, users)
    good.mf_user.to(torch.bfloat16)
    assert not can(good, users)
    f = lambda *s: torch.zeros(*s, device="cuda")  # noqa: E731
    with pytest.raises(RuntimeError, match="multiple of 8"):
        ext.neumf_fwd(users, users, [f(NU, 12), f(NI, 12), f(NU, 8), f(NI, 8)],
                      [f(8, 16)], [f(8)], f(1, 20), f(1), None, None, False)
