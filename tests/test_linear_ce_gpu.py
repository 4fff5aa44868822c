"""Fused linear + cross-entropy HIP kernels (ops/csrc/lce_ops.hip) against
the formulas in float64 on the bf16-rounded h, W, b the kernels see.

Loss bound per labelled row (u = 2^-24, K terms per dot product, p the
softmax weights of the row, so d lse / d z_v = p_v):

  pre-activation  e_v = (K + 2) u (|b_v| + sum_k |h_k w_vk|)
  log2 domain     z * log2(e) and back: 4 u |z_v|
  lse             sum_v p_v (e_v + 4 u |z_v|), first order (the terms are
                  ~1e-5, the second order is far below one ulp)
  sum of exp2     relative error of the sum, which is the absolute error of
                  its log: exp2 to 2 ulp (4 u) per term; 4 + 4 additions in a
                  tile (four columns of a lane, four dpp steps); per tile of
                  a split (8) a rescale (exp2 4 u, product u) and an
                  addition; per split the same three once more in the
                  combine: (4 + 8 + 6 * 8 + 6 * splits) u
  loss            lse error + e_t + 8 u (|lse| + |z_t|), the last for the
                  rounding of M, log2(sum), their sum and the product by ln 2

Gradients pass through bf16 dz and library GEMMs with bf16 outputs: their
max error is held to twice that of the torch bf16 composite on the same
inputs against the same reference (the rule of test_fused_lstm_gpu.py)."""
import pytest
import torch

from tests.linear_ce_ref import make_inputs, reference

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


@pytest.fixture
def ext():
    from autodist_amd.ops import api
    if not api.has_gpu_ops():
        pytest.skip("no GPU ops")
    return api.ext()


def _run(h, w, b, labels, g=None, **kw):
    from autodist_amd.ops.fused_linear_ce import fused_linear_cross_entropy
    h, w = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True) if b is not None else None
    out = fused_linear_cross_entropy(h, w, b, labels, **kw)
    (out if g is None else (out * g).sum()).backward()
    res = {"loss": out.detach(), "dh": h.grad, "dW": w.grad}
    if b is not None:
        res["db"] = b.grad
    return out.grad_fn, res


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("table", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,V,K,labelled", [(5, 40, 32, 2), (70, 200, 96, 66),
                                            (200, "split+1", 1024, 100)])
def test_linear_ce_vs_float64(ext, monkeypatch, N, V, K, labelled, table,
                              bias):
    V = ext.LCE_SPLIT_COLS + 1 if V == "split+1" else V
    h, w, b, labels = make_inputs(N, V, K, labelled, seed=N + V + K)
    keep = labels != -100
    assert keep.sum() == labelled and not keep[0] and not keep[-1]
    assert (labels == V - 1).any()
    g = torch.rand(N, generator=torch.Generator().manual_seed(N)) + 0.5
    b = b if bias else None
    ref = reference(h, w, b, labels, g)
    args = [x.cuda() if x is not None else None
            for x in (h.bfloat16(), w.to(table), b, labels, g)]

    fn, got = _run(*args, reduction="none")
    assert type(fn).__name__ == "_LinearCEFnBackward"
    _, again = _run(*args, reduction="none")
    for k in got:                       # no atomics: the same bits every run
        assert torch.equal(got[k], again[k]), k
    assert not got["dh"][~keep.cuda()].any() and not got["loss"][0]
    monkeypatch.setenv("AUTODIST_LINEAR_CE", "torch")
    fn, comp = _run(*args, reduction="none")
    assert type(fn).__name__ != "_LinearCEFnBackward"

    bd = b.double().abs() if bias else torch.zeros(V, dtype=torch.float64)
    z, lse, zt = ref["z"], ref["lse"], ref["zt"]
    e = ((K + 2) * U * (bd + h.double().abs() @ w.double().abs().t())
         + 4 * U * z.abs())
    p = (z - lse[:, None]).exp()
    e_t = e.gather(1, labels.clamp(min=0)[:, None])[:, 0]
    splits = -(-V // ext.LCE_SPLIT_COLS)
    tol = ((p * e).sum(1) + e_t + (60 + 6 * splits) * U
           + 8 * U * (lse.abs() + zt.abs()))
    err = (got["loss"].double().cpu() - ref["loss"]).abs()
    print(f"loss: max err {err.max():.3e}, max err / bound "
          f"{(err / tol).max():.3f}, composite "
          f"{(comp['loss'].double().cpu() - ref['loss']).abs().max():.3e}")
    assert (err <= tol).all(), f"loss: {int((err > tol).sum())} rows outside"
    worst = []
    for k in ("dh", "dW", "db")[:2 + bias]:
        e_k = (got[k].double().cpu() - ref[k]).abs().max().item()
        e_c = (comp[k].double().cpu() - ref[k]).abs().max().item()
        print(f"{k}: kernels {e_k:.3e} composite {e_c:.3e}")
        if not e_k <= 2 * e_c:
            worst.append((k, e_k, e_c))
    assert not worst, f"error above 2x the torch bf16 composite: {worst}"


@pytest.mark.parametrize("N,labelled,roomy,tight", [(70, 66, 69, 40),
                                                    (200, 60, 64, 33)])
def test_max_rows(ext, N, labelled, roomy, tight):
    """A bound at or above the labelled count changes no bit (the second
    case also changes the number of row blocks, 4 to 1); a bound below it
    equals a call without a bound whose surplus labels were set to -100 by
    hand."""
    h, w, b, labels = make_inputs(N, 200, 96, labelled, seed=7)
    args = [h.bfloat16().cuda(), w.cuda(), b.cuda()]
    _, full = _run(*args, labels.cuda())
    _, room = _run(*args, labels.cuda(), max_rows=roomy)
    by_hand = labels.clone()
    by_hand[(labels != -100).nonzero()[tight:, 0]] = -100
    _, cut = _run(*args, labels.cuda(), max_rows=tight)
    _, cut_ref = _run(*args, by_hand.cuda())
    assert full["loss"].isfinite() and cut["loss"] != full["loss"]
    differ = [(name, k) for name, a, c in (("roomy", room, full),
                                           ("tight", cut, cut_ref))
              for k in full if not torch.equal(a[k], c[k])]
    assert not differ, differ


def test_nothing_labelled(ext):
    from autodist_amd.ops.fused_linear_ce import fused_linear_cross_entropy
    h, w, b, labels = (x.cuda() for x in make_inputs(70, 200, 96, 66, seed=3))
    labels[:] = -100
    h = h.bfloat16()
    assert fused_linear_cross_entropy(h, w, b, labels).isnan()
    rows = fused_linear_cross_entropy(h, w, b, labels, reduction="none")
    assert rows.shape == (70,) and not rows.any()


def test_binding_refusals(ext):
    from autodist_amd.ops.fused_linear_ce import can_use_lce_kernels
    labels = torch.zeros(4, dtype=torch.long, device="cuda")
    wide = torch.randn(4, 1056, device="cuda").bfloat16()
    for K, h, msg in [(40, wide[:, :40].contiguous(), "multiple of 32"),
                      (1056, wide, "multiple of 32"),
                      (64, wide[:, :128:2], "contiguous")]:
        w = torch.randn(50, K, device="cuda")
        assert not can_use_lce_kernels(h, w, None)
        with pytest.raises(RuntimeError, match=msg):
            ext.lce_compact(h, labels, -100, 4)
    h = wide[:, :64].contiguous()
    with pytest.raises(RuntimeError, match="int64"):
        ext.lce_compact(h, labels.int(), -100, 4)
    w = torch.randn(50, 64, device="cuda")
    assert can_use_lce_kernels(h, w, None)
    assert not can_use_lce_kernels(h, w.cpu(), None)
    assert not can_use_lce_kernels(h, wide[:, :128:2], None)  # bf16 in place
    with torch.autocast("cuda", dtype=torch.float16):
        assert not can_use_lce_kernels(h.float(), w, None)


def test_label_out_of_range_is_nan(ext):
    from autodist_amd.ops.fused_linear_ce import fused_linear_cross_entropy
    h, w, b, labels = (x.cuda() for x in make_inputs(5, 40, 32, 2, seed=4))
    labels[2] = 40
    rows = fused_linear_cross_entropy(h.bfloat16(), w, b, labels,
                                      reduction="none")
    assert rows[2].isnan() and rows[[0, 1, 3, 4]].isfinite().all()


def _graph_names(fn, seen):
    if fn is not None and fn not in seen:
        seen[fn] = type(fn).__name__
        for nxt, _ in fn.next_functions:
            _graph_names(nxt, seen)
    return set(seen.values())


def test_bert_mlm_loss(ext, monkeypatch):
    from autodist_amd.models.bert import BertConfig, BertForPreTraining
    torch.manual_seed(0)
    model = BertForPreTraining(BertConfig(
        vocab_size=1000, hidden=64, layers=1, heads=2, intermediate=128,
        max_seq=32)).cuda().eval()
    ids = torch.randint(0, 1000, (4, 32), device="cuda")
    labels = torch.where(torch.rand(4, 32, device="cuda") < 0.5, ids, -100)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = model.loss(ids, labels)
    assert "_LinearCEFnBackward" in _graph_names(loss.grad_fn, {})
    loss.backward()
    grad = model.bert.tok_emb.weight.grad
    assert grad.dtype == torch.float32 and grad.isfinite().all()
    loss_fp32 = model.loss(ids, labels).item()
    monkeypatch.setenv("AUTODIST_LINEAR_CE", "torch")
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss_torch = model.loss(ids, labels)
    assert "_LinearCEFnBackward" not in _graph_names(loss_torch.grad_fn, {})
    print(f"loss fp32 {loss_fp32:.6f} kernels {loss.item():.6f} "
          f"torch bf16 {loss_torch.item():.6f}")
    assert abs(loss.item() - loss_fp32) <= 2 * abs(loss_torch.item()
                                                   - loss_fp32)
