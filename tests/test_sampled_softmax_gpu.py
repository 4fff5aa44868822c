"""Sampled softmax HIP kernels (ops/csrc/ssm_ops.hip) against the formulas in
float64 on the bf16-rounded h and table rows the kernels see.

Loss bound per row (u = 2^-24, P terms per dot product, p the softmax
weights of the row over (z0, z), so d lse / d z_s = p_s):

  pre-activation  e_s = (P + 2) u (|off_s| + sum_k |h_k w_sk|), e_0 alike
  log2 domain     z * log2(e) and back: 4 u |z_s|
  lse             sum_s p_s (e_s + 4 u |z_s|), first order (the terms are
                  ~1e-5, the second order is far below one ulp)
  sum of exp2     exp2 to 2 ulp, S + 1 terms added in 8 + tiles + splits
                  steps, log2 to 1 ulp: (32 + S / 64) u absolute
  loss            lse error + e_0 + 8 u (|lse| + |z0|)

Gradients pass through bf16 dz and library GEMMs with bf16 outputs: their
max error is held to twice that of the torch bf16 composite on the same
inputs against the same reference (the rule of test_fused_lstm_gpu.py).

The sparse gradient is coalesced by a plain loop that adds duplicates in
index order, as coalesce() does: on the ROCm stack this was written on,
torch's GPU coalesce() returns wrong sums for 512-wide rows (583 x 512
values over 300 rows: max error 6.6 against a float64 index_add, 4e37 in
another draw; exact at widths 32, 96, 256 and 500), so it is also asserted
only below that width."""
import pytest
import torch

from tests.sampled_softmax_ref import make_inputs, reference

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
V = 300


@pytest.fixture
def ext():
    from autodist_amd.ops import api
    if not api.has_gpu_ops():
        pytest.skip("no GPU ops")
    return api.ext()


def _run(h, w, b, t, c, lq_t, lq_s, g, sparse_grad=False):
    from autodist_amd.ops.sampled_softmax import sampled_softmax_loss
    h, w = h.clone().requires_grad_(True), w.clone().requires_grad_(True)
    b = b.clone().requires_grad_(True) if b is not None else None
    rows = sampled_softmax_loss(h, w, b, t, c, lq_t, lq_s, reduction="none",
                                sparse_grad=sparse_grad)
    (rows * g).sum().backward()
    out = {"loss": rows.detach(), "dH": h.grad, "dW": w.grad}
    if b is not None:
        out["db"] = b.grad
    return rows.grad_fn, out


@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("table", [torch.float32, torch.bfloat16],
                         ids=["fp32", "bf16"])
@pytest.mark.parametrize("N,S,P", [(5, 40, 32), (35, 200, 96),
                                   (70, "split+1", 512)])
def test_sampled_softmax_vs_float64(ext, monkeypatch, N, S, P, table, bias):
    S = ext.SSM_SPLIT_COLS + 1 if S == "split+1" else S
    h, w, b, t, c, lq_t, lq_s = make_inputs(N, S, P, V, seed=N + S + P)
    assert (t[:, None] == c[None, :]).any(1).float().mean() > 0.5
    assert c.unique().numel() < S
    g = torch.rand(N, generator=torch.Generator().manual_seed(N)) + 0.5
    h, w = h.bfloat16(), w.bfloat16()
    b = b if bias else None
    ref = reference(h, w, b, t, c, lq_t, lq_s, g)
    ref["dW"] = torch.zeros(V, P, dtype=torch.float64).index_add_(
        0, torch.cat([c, t]), ref.pop("dW_rows"))
    args = [x.cuda() if x is not None else None
            for x in (h, w.to(table), b, t, c, lq_t, lq_s, g)]

    fn, got = _run(*args)
    assert type(fn).__name__ == "_SampledSoftmaxFnBackward"
    _, again = _run(*args)
    for k in got:                       # no atomics: the same bits every run
        assert torch.equal(got[k], again[k]), k
    if table == torch.float32:          # bf16 values coalesce in bf16
        _, sp = _run(*args, sparse_grad=True)
        ids, vals = sp["dW"]._indices()[0].cpu(), sp["dW"]._values().cpu()
        assert sp["dW"].is_sparse and not sp["dW"].is_coalesced()
        assert torch.equal(ids, torch.cat([c, t]))
        dense = torch.zeros(V, P)
        for i, v in zip(ids.tolist(), vals):    # coalesce: in index order
            dense[i] += v
        assert torch.equal(dense, got["dW"].cpu())
        if P < 512:     # torch's own GPU coalesce, where it can be trusted
            assert torch.equal(sp["dW"].coalesce().to_dense(), got["dW"])
    monkeypatch.setenv("AUTODIST_SAMPLED_SOFTMAX", "torch")
    fn, comp = _run(*args)
    assert type(fn).__name__ != "_SampledSoftmaxFnBackward"

    hd, wd = h.double(), w.double()
    bd = b.double() if bias else torch.zeros(V, dtype=torch.float64)
    z = torch.cat([ref["z0"][:, None], ref["z"]], 1)
    off = torch.cat([(bd[t] - lq_t).abs()[:, None],
                     (bd[c] - lq_s).abs().expand(N, S)], 1)
    dots = torch.cat([(hd.abs() * wd[t].abs()).sum(1, keepdim=True),
                      hd.abs() @ wd[c].abs().t()], 1)
    e = (P + 2) * U * (off + dots) + 4 * U * z.abs().nan_to_num(posinf=0.0)
    p = (z - ref["lse"][:, None]).exp()
    tol = ((p * e).sum(1) + e[:, 0] + (32 + S / 64) * U
           + 8 * U * (ref["lse"].abs() + ref["z0"].abs()))
    err = (got["loss"].double().cpu() - ref["loss"]).abs()
    print(f"loss: max err {err.max():.3e}, max err / bound "
          f"{(err / tol).max():.3f}, composite "
          f"{(comp['loss'].double().cpu() - ref['loss']).abs().max():.3e}")
    assert (err <= tol).all(), f"loss: {int((err > tol).sum())} rows outside"
    worst = []
    for k in got:
        if k == "loss":
            continue
        e_k = (got[k].double().cpu() - ref[k]).abs().max().item()
        e_c = (comp[k].double().cpu() - ref[k]).abs().max().item()
        print(f"{k}: kernels {e_k:.3e} composite {e_c:.3e}")
        if not e_k <= 2 * e_c:
            worst.append((k, e_k, e_c))
    assert not worst, f"error above 2x the torch bf16 composite: {worst}"


def test_all_candidates_removed_is_exact(ext):
    """Row 0's 16 candidates are all its own target: lse == z0 exactly."""
    N, S, P = 5, 16, 32
    h, w, b, t, c, lq_t, lq_s = (x.cuda() for x in
                                 make_inputs(N, S, P, V, seed=1))
    c[:] = t[0]
    t[1:] = (t[0] + 1 + torch.arange(N - 1, device="cuda")) % V
    h = h.bfloat16()
    wg, wt, off, off0 = ext.ssm_prep(w, b, c, t, lq_s, lq_t)
    loss, lse2, z0 = ext.ssm_fwd(h, wg, wt, off, off0, c, t)
    dz, dz0, db = ext.ssm_bwd(h, wg, off, c, t, lse2, z0,
                              torch.ones(N, device="cuda"))
    assert loss[0].item() == 0.0 and dz0[0].item() == 0.0
    assert not dz[0].any() and not dz[:, S:].any()
    assert (loss[1:] > 0).all() and dz[1:, :S].float().min() > 0


def test_binding_refusals(ext):
    from autodist_amd.ops.sampled_softmax import can_use_ssm_kernels
    N, S = 4, 8
    h, w, b, t, c, lq_t, lq_s = (x.cuda() for x in
                                 make_inputs(N, S, 40, V, seed=2))
    assert not can_use_ssm_kernels(h.bfloat16(), w, b)
    with pytest.raises(RuntimeError, match="multiple of 32"):
        ext.ssm_prep(w, b, c, t, lq_s, lq_t)
    w64 = torch.randn(V, 64, device="cuda")
    wg, wt, off, off0 = ext.ssm_prep(w64, b, c, t, lq_s, lq_t)
    h2 = torch.randn(N, 128, device="cuda").bfloat16()[:, ::2]
    with pytest.raises(RuntimeError, match="contiguous"):
        ext.ssm_fwd(h2, wg, wt, off, off0, c, t)
    with pytest.raises(RuntimeError, match="S <= 2"):
        ext.ssm_prep(w64, b, c[:0], t, lq_s[:0], lq_t)
