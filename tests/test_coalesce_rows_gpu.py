"""Sort-free deterministic coalesce (ops/csrc/sparse_ops.hip) against a
sequential CPU loop, bit for bit.

Reference: sv = vals * scale in fp32, then rows added in ascending input
position into the row of their id, first addend copied. Values have exponents
spread over 2^-12 .. 2^12, so another summation order changes bits. Every
comparison is torch.equal; no tolerance is involved, except in the engine
case's comparison with the sorting path, which uses the Adagrad tolerance of
tests/test_sparse_apply_gpu.py.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

ADAGRAD_ATOL = 1e-5  # tests/test_sparse_apply_gpu.py


@pytest.fixture(scope="module")
def api():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodist_amd.ops import api as ops_api
    assert ops_api.has_gpu_ops()
    assert hasattr(ops_api.ext(), "coalesce_rows_ranked")
    return ops_api


def _vals(n, dim, gen):
    expo = torch.randint(-12, 13, (n, dim), generator=gen).float()
    return torch.randn(n, dim, generator=gen) * torch.exp2(expo)


def _zipf_ids(rows, n, gen):
    u = torch.rand(n, generator=gen)
    return (rows ** u - 1).long().clamp_(0, rows - 1)


def _reference(ids, vals, scale):
    sv = vals * torch.tensor(scale, dtype=torch.float32)
    rows = {}
    for i, r in enumerate(ids.tolist()):
        rows[r] = sv[i].clone() if r not in rows else rows[r] + sv[i]
    uniq = sorted(rows)
    return (torch.tensor(uniq, dtype=torch.int64),
            torch.stack([rows[r] for r in uniq]))


def _ids_for(kind, rows, n, gen):
    if kind == "rand":
        return torch.randint(0, rows, (n,), generator=gen)
    if kind == "edges":
        return torch.tensor([0, 31, 32])[torch.randint(0, 3, (n,),
                                                       generator=gen)]
    if kind == "desc":
        return torch.arange(rows - 1, -1, -1)
    if kind == "one":
        return torch.full((n,), rows // 2)
    return _zipf_ids(rows, n, gen)


CASES = (
    [("rand", 1, 1, 1, 1.0), ("edges", 33, 40, 3, 1.0),
     ("desc", 64, 64, 4, 1.0)]
    + [("rand", 1000, 257, d, 1.0) for d in (1, 3, 4, 64, 100, 128)]
    + [("one", 50, n, 8, 1.0) for n in (2, 64, 65, 300)]
    + [("zipf", 5000, 4096, 64, 1.0), ("rand", 100_003, 513, 4, 1.0),
       ("rand", 2 ** 22 + 5, 1000, 4, 1.0),
       ("rand", 1000, 257, 100, 0.3), ("zipf", 5000, 4096, 64, 1.0 / 7)])


@pytest.mark.parametrize("kind,rows,n,dim,scale", CASES)
def test_matches_sequential_sum(api, kind, rows, n, dim, scale):
    gen = torch.Generator().manual_seed(rows + 7 * n + dim)
    ids, vals = _ids_for(kind, rows, n, gen), _vals(n, dim, gen)
    want_u, want_o = _reference(ids, vals, scale)
    m = want_u.shape[0]
    got_u, got_o = api.coalesce_rows_ranked(ids.cuda(), vals.cuda(), rows,
                                            scale)
    assert torch.equal(got_u.cpu(), want_u)
    assert torch.equal(got_o.cpu(), want_o)
    pad_u, pad_o, count = api.coalesce_rows_ranked(
        ids.cuda(), vals.cuda(), rows, scale, exact=False)
    assert pad_u.shape == (n,) and pad_o.shape == (n, dim)
    assert count.dtype == torch.int32 and int(count) == m
    assert torch.equal(pad_u[:m].cpu(), want_u)
    assert torch.equal(pad_o[:m].cpu(), want_o)
    assert bool((pad_u[m:] == -1).all()) and bool((pad_o[m:] == 0).all())
    if kind == "zipf":  # run to run: the same bits every time
        for _ in range(2):
            again = api.coalesce_rows_ranked(ids.cuda(), vals.cuda(), rows,
                                             scale)
            assert torch.equal(again[1], got_o)


def test_workspace_is_clean_for_the_next_call(api):
    """Two calls on one table height with different ids: a bitmap that was
    not cleared would leak the first call's ids into the second."""
    gen = torch.Generator().manual_seed(11)
    rows = 70_001
    for n in (300, 200):
        ids, vals = _ids_for("rand", rows, n, gen), _vals(n, 4, gen)
        want_u, want_o = _reference(ids, vals, 1.0)
        got_u, got_o = api.coalesce_rows_ranked(ids.cuda(), vals.cuda(), rows)
        assert torch.equal(got_u.cpu(), want_u)
        assert torch.equal(got_o.cpu(), want_o)


@pytest.mark.parametrize("opt", ["SGD", "Adagrad"])
def test_padded_pair_applies_like_the_exact_pair(api, opt):
    gen = torch.Generator().manual_seed(12)
    rows, n, dim = 300, 257, 12
    ids = _ids_for("zipf", rows, n, gen).cuda()
    vals = torch.randn(n, dim, generator=gen).cuda()
    hyper = {"lr": 0.05, "lr_decay": 0.1, "eps": 1e-10}
    results = []
    for exact in (True, False):
        table = torch.linspace(-1, 1, rows * dim).view(rows, dim).cuda()
        state = {"step": torch.tensor(2.0),
                 "sum": torch.full((rows, dim), 0.25).cuda()}
        u, o = api.coalesce_rows_ranked(ids, vals, rows, exact=exact)[:2]
        assert exact or u.shape[0] == n
        assert api.fused_sparse_apply(opt, table, u, o, state, hyper)
        results.append((table, state["sum"]))
    assert torch.equal(results[0][0], results[1][0])
    assert torch.equal(results[0][1], results[1][1])


def _engine_steps(monkeypatch, mode):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.resource_spec import ResourceSpec
    from autodist_amd.strategy import Parallax
    monkeypatch.setenv("AUTODIST_SPARSE_COALESCE", mode)
    torch.manual_seed(5)
    emb = torch.nn.Embedding(40, 8, sparse=True).cuda()
    g = GraphItem()
    g.extend_model(emb)
    opt = torch.optim.Adagrad(emb.parameters(), lr=0.1)
    g.extend_optimizer_info(opt)
    engine = DistributedEngine(g, Parallax().build(g, ResourceSpec()), rank=0,
                               world_size=1,
                               device=torch.device("cuda", 0)).setup()
    gen = torch.Generator().manual_seed(6)
    ids = torch.tensor([3, 17, 3, 39, 0, 17, 3, 3], device="cuda")
    weight = _vals(8, 8, gen).cuda() / 4096
    for _ in range(2):
        opt.zero_grad()
        (emb(ids) * weight).sum().backward()
        opt.step()
    engine.drain()
    engine.teardown()
    return emb.weight.detach().clone()


def test_engine_step_is_bit_reproducible(api, monkeypatch):
    first = _engine_steps(monkeypatch, "ranked")
    second = _engine_steps(monkeypatch, "ranked")
    sorting = _engine_steps(monkeypatch, "unique")
    assert torch.equal(first, second)
    assert (first - sorting).abs().max().item() <= ADAGRAD_ATOL
