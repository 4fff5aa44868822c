"""Fused row-wise optimizer apply (sparse_apply_rows_kernel) vs the torch
composite it replaces.

Reference: apply_sparse_rows_torch on cloned tensors. Inputs have |values|
<= 1; tolerances are the dense kernels' own (tests/test_gpu_kernels.py):
1e-6 for SGD, 1e-5 for Adagrad and Adam. Rows the call must not touch —
rows not listed, and rows of the larger table outside the shard — are held
to torch.equal with their value before the call.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

TABLE_ROWS = 600       # the full table; the shard is a narrow() view of it
SHARD_ROWS = 300

HYPER = {
    "SGD": {"lr": 0.05},
    "Adagrad": {"lr": 0.05, "lr_decay": 0.1, "eps": 1e-10},
    "Adam": {"lr": 0.01, "betas": (0.9, 0.999), "eps": 1e-8},
}
ATOL = {"SGD": 1e-6, "Adagrad": 1e-5, "Adam": 1e-5}


@pytest.fixture(scope="module")
def gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from autodist_amd.ops import api as ops_api
    assert ops_api.has_gpu_ops()
    return torch.device("cuda", 0)


def _uniform(shape, gen, lo=-1.0, hi=1.0):
    return (torch.rand(shape, generator=gen) * (hi - lo) + lo).cuda()


def _make_state(opt, dim, gen):
    if opt == "SGD":
        return {}
    step = torch.tensor(2.0)  # host-side counter, as make_state builds it
    if opt == "Adagrad":
        return {"step": step,
                "sum": _uniform((SHARD_ROWS, dim), gen, 0.0, 1.0)}
    return {"step": step,
            "exp_avg": _uniform((SHARD_ROWS, dim), gen),
            "exp_avg_sq": _uniform((SHARD_ROWS, dim), gen, 0.0, 1.0)}


def _ids(n, row_base, gen):
    """Global row ids (unique, unsorted). n=257 covers the shard's first and
    last row and one id just outside each end (which must be skipped)."""
    first, last = row_base, row_base + SHARD_ROWS - 1
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    if n == 1:
        return torch.tensor([last])
    edge = torch.tensor([first, last, first - 1, last + 1])
    inner = torch.randperm(SHARD_ROWS - 2, generator=gen)[:n - 4] + first + 1
    ids = torch.cat([edge, inner])
    return ids[torch.randperm(n, generator=gen)]


def _clone_state(state):
    return {k: v.clone() for k, v in state.items()}


@pytest.mark.parametrize("row_base", [0, 137])
@pytest.mark.parametrize("n", [0, 1, 257])
@pytest.mark.parametrize("dim", [4, 6, 64, 200])
@pytest.mark.parametrize("opt", ["SGD", "Adagrad", "Adam"])
def test_sparse_apply_matches_torch(gpu, opt, dim, n, row_base):
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    gen = torch.Generator().manual_seed(1000 * dim + 10 * n + row_base)
    hyper = HYPER[opt]
    table = _uniform((TABLE_ROWS, dim), gen)
    state = _make_state(opt, dim, gen)
    ids = _ids(n, row_base, gen).cuda()
    grads = _uniform((n, dim), gen)
    new_rows = torch.full((n, dim), 7.0, device="cuda")

    table0, state0 = table.clone(), _clone_state(state)
    table_ref, state_ref = table.clone(), _clone_state(state)
    new_rows_ref = new_rows.clone()
    apply_mod.apply_sparse_rows_torch(
        opt, table_ref.narrow(0, row_base, SHARD_ROWS), ids, grads, state_ref,
        hyper, row_base=row_base, new_rows=new_rows_ref)

    shard = table.narrow(0, row_base, SHARD_ROWS)
    assert shard.data_ptr() == table.data_ptr() + row_base * dim * 4
    assert ops_api.fused_sparse_apply(opt, shard, ids, grads, state, hyper,
                                      row_base=row_base, new_rows=new_rows)
    torch.cuda.synchronize()

    atol = ATOL[opt]
    err = (table - table_ref).abs().max().item()
    print(f"{opt} D={dim} n={n} base={row_base}: max |param err| {err:.3e}")
    assert err <= atol
    for k in state:
        if k == "step":
            assert float(state[k]) == float(state_ref[k]) == 3.0
            continue
        serr = (state[k] - state_ref[k]).abs().max().item()
        print(f"  state {k}: max err {serr:.3e}")
        assert serr <= atol
    # stray writes: every row not listed keeps its bits, in the shard, in the
    # rest of the table, and in the state
    local = ids - row_base
    inside = (local >= 0) & (local < SHARD_ROWS)
    touched_table = torch.zeros(TABLE_ROWS, dtype=torch.bool, device="cuda")
    touched_table[ids[inside]] = True
    assert int(touched_table.sum()) == int(inside.sum())
    assert torch.equal(table[~touched_table], table0[~touched_table])
    touched_shard = touched_table[row_base:row_base + SHARD_ROWS]
    for k in state:
        if k != "step":
            assert torch.equal(state[k][~touched_shard],
                               state0[k][~touched_shard])
    if n:
        assert not torch.equal(table[touched_table], table0[touched_table])
    # pull payload: the updated rows, exactly; skipped ids leave theirs alone
    assert torch.equal(new_rows[inside], shard[local[inside]])
    assert torch.equal(new_rows[~inside],
                       torch.full_like(new_rows[~inside], 7.0))
    if n == 257:
        assert int((~inside).sum()) == 2


def test_sparse_apply_without_new_rows_and_unsupported(gpu):
    """new_rows is optional; classes / flags without a kernel return False
    and leave everything untouched."""
    from autodist_amd.ops import api as ops_api
    gen = torch.Generator().manual_seed(3)
    p = _uniform((50, 8), gen)
    ids = torch.tensor([0, 49, 7], device="cuda")
    g = _uniform((3, 8), gen)
    p0 = p.clone()
    assert ops_api.fused_sparse_apply("SGD", p, ids, g, {}, {"lr": 0.5})
    want = p0.clone()
    want[ids] -= 0.5 * g
    assert torch.allclose(p, want, atol=1e-6)
    p1 = p.clone()
    assert not ops_api.fused_sparse_apply("RMSprop", p, ids, g, {},
                                          {"lr": 0.5})
    assert not ops_api.fused_sparse_apply("SGD", p, ids, g, {},
                                          {"lr": 0.5, "momentum": 0.9})
    assert not ops_api.fused_sparse_apply("SGD", p, ids.to(torch.int32), g,
                                          {}, {"lr": 0.5})
    assert not ops_api.fused_sparse_apply("SGD", p.t(), ids, g, {},
                                          {"lr": 0.5})
    assert torch.equal(p, p1)


def test_apply_sparse_rows_dispatch_uses_hip(gpu, monkeypatch):
    """apply_sparse_rows on GPU must route through the HIP kernel and match
    the CPU torch reference."""
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    calls = []
    real = ops_api.ext().sparse_apply_rows

    class _Spy:
        def __getattr__(self, name):
            return getattr(ops_api._ext, name)

        @staticmethod
        def sparse_apply_rows(*args):
            calls.append(args[0])
            return real(*args)

    monkeypatch.setattr(ops_api, "_load", lambda: _Spy())
    gen = torch.Generator().manual_seed(4)
    p_gpu = _uniform((100, 16), gen)
    ids = torch.tensor([3, 99, 0, 41], device="cuda")
    g_gpu = _uniform((4, 16), gen)
    p_cpu = p_gpu.cpu()
    hyper = {"lr": 0.05, "lr_decay": 0.0, "eps": 1e-10}
    st_gpu = apply_mod.make_state("Adagrad", p_gpu, hyper)
    st_cpu = apply_mod.make_state("Adagrad", p_cpu, hyper)
    for _ in range(2):
        apply_mod.apply_sparse_rows("Adagrad", p_gpu, ids, g_gpu, st_gpu,
                                    hyper)
        apply_mod.apply_sparse_rows("Adagrad", p_cpu, ids.cpu(), g_gpu.cpu(),
                                    st_cpu, hyper)
    assert calls == [1, 1]
    assert float(st_gpu["step"]) == 2.0
    assert torch.allclose(p_gpu.cpu(), p_cpu, atol=1e-5)
    assert torch.allclose(st_gpu["sum"].cpu(), st_cpu["sum"], atol=1e-5)
