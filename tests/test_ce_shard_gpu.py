"""Vocab-sharded cross-entropy kernels (ce_shard_stats / _combine / _bwd)
against float64, and the public path through VocabParallelProjection.loss.

Error model, as in tests/test_fused_ln_gpu.py: loss rows 2^-20 * max(1,
row_max * log2e); bf16-stored dlogits 2^-7 * |ref| + 1e-4 * |dloss_row|;
dbias the column sum of those bounds plus L * 2^-24 * sum|terms|, L the
sequential adds of the kernel (rows of a chunk, then the chunks, + the
roundings inside a term)."""
import math
import socket

import pytest
import torch
import torch.distributed as dist

pytestmark = pytest.mark.gpu

U24 = 2.0 ** -24
BF16 = 2.0 ** -7


@pytest.fixture
def ext():
    from autodist_amd.ops import api
    if not api.has_gpu_ops():
        pytest.skip("no GPU ops")
    return api.ext()


def _within(name, got, ref, tol):
    err = (got.double() - ref).abs()
    bad = ~(err <= tol.expand_as(err))
    assert not bad.any(), (
        f"{name}: {int(bad.sum())} of {bad.numel()} outside the bound, "
        f"max err {err.max().item():.3e}")


def _shard(full, a, b, layout):
    """Columns [a, b) as the kernels' input: contiguous (odd widths leave
    rows 2-byte aligned: scalar width) or in a row stride rounded up to 8
    (vector width, ragged row end when the width is no multiple of 8)."""
    if layout == "contig":
        return full[:, a:b].contiguous()
    buf = torch.zeros(full.shape[0], (b - a + 7) // 8 * 8, dtype=full.dtype,
                      device=full.device)
    buf[:, :b - a] = full[:, a:b]
    return buf[:, :b - a]


def _run(ext, logits, targets, dloss, bounds, layout):
    shards = [_shard(logits, a, b, layout) for a, b in bounds]
    stats = torch.stack([ext.ce_shard_stats(s, targets, a)
                         for s, (a, _) in zip(shards, bounds)])
    loss, lse2 = ext.ce_shard_combine(stats)
    outs = [ext.ce_shard_bwd(s, targets, a, lse2, dloss)
            for s, (a, _) in zip(shards, bounds)]
    for (dl, _), s in zip(outs, shards):
        assert dl.stride() == s.stride() and dl.dtype == torch.bfloat16
    return (loss, torch.cat([dl for dl, _ in outs], 1),
            torch.cat([db for _, db in outs]))


@pytest.mark.parametrize("layout", ["contig", "padded"])
@pytest.mark.parametrize("many_rows", [False, True], ids=["n1", "chunks"])
@pytest.mark.parametrize("nshards", [3, 1])
def test_ce_shard_kernels_vs_float64(ext, nshards, many_rows, layout):
    S, R = ext.CE_STRIP_COLS, ext.CE_BWD_ROWS
    # below one 16 B vector | exactly one strip | a strip + an odd remainder
    widths = [3, S, S + 37] if nshards == 3 else [S + 37]
    N = R + 6 if many_rows else 1      # two row chunks, ragged second
    V = sum(widths)
    ends = torch.tensor(widths).cumsum(0).tolist()
    bounds = list(zip([0] + ends[:-1], ends))
    g = torch.Generator(device="cuda").manual_seed(V + N)
    logits = torch.randn(N, V, generator=g, device="cuda")
    logits = (logits * (80.0 / logits.abs().max())).bfloat16()
    targets = torch.randint(0, V, (N,), generator=g, device="cuda")
    dloss = torch.tensor([1.0, 0.5, 0.0, -2.0, 3.0, 1.0 / 7, 0.25],
                         device="cuda").repeat(N // 7 + 1)[:N].contiguous()
    if many_rows:
        logits[0] = 60.0                   # all equal: loss = ln V
        targets[2], targets[3] = 0, V - 1
    loss, dlog, dbias = _run(ext, logits, targets, dloss, bounds, layout)

    ld = logits.double()
    lsm = torch.log_softmax(ld, dim=1)
    loss_ref = -lsm.gather(1, targets[:, None])[:, 0]
    if many_rows:
        assert abs(loss_ref[0].item() - math.log(V)) < 1e-12
    row_max = ld.max(1).values.abs()
    _within("loss", loss, loss_ref,
            2.0 ** -20 * (row_max * math.log2(math.e)).clamp_min(1.0))
    d_ref = lsm.exp()
    d_ref[torch.arange(N), targets] -= 1.0
    d_ref = d_ref * dloss.double()[:, None]
    tol_d = BF16 * d_ref.abs() + 1e-4 * dloss.double().abs()[:, None]
    assert torch.isfinite(dlog.float()).all()
    _within("dlogits", dlog, d_ref, tol_d)
    L = min(N, R) + -(-N // R) + 4
    _within("dbias", dbias, d_ref.sum(0),
            tol_d.sum(0) + L * U24 * d_ref.abs().sum(0))


@pytest.mark.parametrize("layout", ["contig", "padded"])
def test_ce_shard_dbias_exact(ext, layout):
    """Every row has the same logits and dloss is integer. Columns 5 and
    V - 1 sit 160 below the maximum: their softmax is exactly 0 in fp32, so
    their dlogits are -dloss on the target rows and 0 elsewhere, and their
    dbias is an exact integer sum over three row chunks. A second run gives
    the same bits in every column (no atomics)."""
    S, R = ext.CE_STRIP_COLS, ext.CE_BWD_ROWS
    N, V = 2 * R + 6, S + 37
    g = torch.Generator(device="cuda").manual_seed(11)
    row = torch.rand(V, generator=g, device="cuda") * 2 + 78
    row[5] = row[V - 1] = -80.0
    logits = row.bfloat16().repeat(N, 1)
    targets = torch.randint(6, V - 1, (N,), generator=g, device="cuda")
    targets[0::3], targets[1::3] = 5, V - 1
    dloss = torch.randint(-4, 5, (N,), generator=g, device="cuda").float()
    loss, dlog, dbias = _run(ext, logits, targets, dloss, [(0, V)], layout)
    for c in (5, V - 1):
        hit = targets == c
        assert torch.equal(dlog[:, c].float(), torch.where(hit, -dloss, 0.0))
        assert dbias[c].item() == -dloss[hit].sum().item()
    _, dlog2, dbias2 = _run(ext, logits, targets, dloss, [(0, V)], layout)
    assert torch.equal(dbias, dbias2) and torch.equal(dlog, dlog2)


@pytest.fixture()
def rccl_world1(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setenv("AUTODIST_FORCE_COLLECTIVES", "1")
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    if not dist.is_initialized():
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        dist.init_process_group(
            "nccl", init_method=f"tcp://127.0.0.1:{port}",
            rank=0, world_size=1)
    yield
    if dist.is_initialized():
        dist.destroy_process_group()


@pytest.mark.parametrize("path", ["hip", "torch", "torch-autocast"])
def test_vocab_parallel_loss_public_path(rccl_world1, monkeypatch, path):
    """loss() under bf16 autocast with backward() outside the autocast
    block runs the HIP function (V = 50 is no multiple of 8: the padded
    GEMM-output view) and matches float64 on the bf16-rounded operands;
    AUTODIST_VOCAB_CE=torch in fp32 keeps the torch chain with today's
    results; under autocast, where the kernels would be chosen, the switch
    alone sends the call to the torch chain (backward inside the block: the
    chain fails outside it)."""
    from autodist_amd.parallel.vocab_parallel import VocabParallelProjection
    torch.manual_seed(9)
    V, D, N = 50, 16, 12
    proj = VocabParallelProjection(V, D, rank=0, world_size=1).cuda()
    with torch.no_grad():
        proj.bias.normal_(std=0.1)
    hidden = torch.randn(N, D, device="cuda", requires_grad=True)
    targets = torch.randint(0, V, (N,), device="cuda")
    if path == "hip":
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = proj.loss(hidden, targets)
        assert type(loss.grad_fn).__name__ == "_VocabParallelCEHipBackward"
        rnd = lambda t: t.detach().bfloat16().double()  # noqa: E731
    elif path == "torch-autocast":
        monkeypatch.setenv("AUTODIST_VOCAB_CE", "torch")
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = proj.loss(hidden, targets)
            assert type(loss.grad_fn).__name__ == "_VocabParallelCEBackward"
            loss.backward()
        assert torch.isfinite(hidden.grad).all()
        return
    else:
        monkeypatch.setenv("AUTODIST_VOCAB_CE", "torch")
        loss = proj.loss(hidden, targets)
        assert type(loss.grad_fn).__name__ == "_VocabParallelCEBackward"
        rnd = lambda t: t.detach().double()  # noqa: E731
    loss.backward()
    assert hidden.grad.dtype == proj.weight.grad.dtype == torch.float32

    h = rnd(hidden).requires_grad_(True)
    w = rnd(proj.weight).requires_grad_(True)
    b = rnd(proj.bias).requires_grad_(True)
    logits = h @ w.t() + b
    logits.retain_grad()
    ref = torch.nn.functional.cross_entropy(logits, targets)
    ref.backward()
    if path == "torch":
        assert abs(loss.item() - ref.item()) < 1e-4
        assert torch.allclose(hidden.grad.double(), h.grad, atol=1e-4)
        assert torch.allclose(proj.weight.grad.double(), w.grad, atol=1e-4)
        assert torch.allclose(proj.bias.grad.double(), b.grad, atol=1e-4)
        return
    assert abs(loss.item() - ref.item()) < 2e-3 * abs(ref.item()) + 1e-3
    # dlogits bound, carried through the sums of the three products; each
    # product leaves its GEMM rounded to bf16
    E = BF16 * logits.grad.abs() + 1e-4 / N
    _within("dhidden", hidden.grad, h.grad,
            BF16 * h.grad.abs() + E @ w.detach().abs())
    _within("dweight", proj.weight.grad, w.grad,
            BF16 * w.grad.abs() + E.t() @ h.detach().abs())
    _within("dbias", proj.bias.grad, b.grad, BF16 * b.grad.abs() + E.sum(0))
