"""The torch composite behind coalesce_rows_ranked (CPU tensors, a missing
extension, non-fp32 values) gives the results of the HIP path: a sequential
sum per id, bit for bit, and the same padded outputs."""
import pytest
import torch

from autodist_amd.ops import api as ops_api
from autodist_amd.parallel.comm import coalesce_rows


@pytest.mark.parametrize("scale", [1.0, 0.3])
def test_fallback_matches_sequential_sum(scale):
    gen = torch.Generator().manual_seed(3)
    n, dim, rows = 200, 5, 37
    ids = torch.randint(0, rows, (n,), generator=gen)
    expo = torch.randint(-12, 13, (n, dim), generator=gen).float()
    vals = torch.randn(n, dim, generator=gen) * torch.exp2(expo)
    sv = vals * torch.tensor(scale, dtype=torch.float32)
    want = {}
    for i, r in enumerate(ids.tolist()):
        want[r] = sv[i].clone() if r not in want else want[r] + sv[i]
    want_u = torch.tensor(sorted(want))
    want_o = torch.stack([want[r] for r in sorted(want)])
    m = want_u.shape[0]
    uniq, out = ops_api.coalesce_rows_ranked(ids, vals, rows, scale)
    assert torch.equal(uniq, want_u) and torch.equal(out, want_o)
    pad_u, pad_o, count = ops_api.coalesce_rows_ranked(ids, vals, rows, scale,
                                                       exact=False)
    assert int(count) == m and count.dtype == torch.int32
    assert torch.equal(pad_u[:m], want_u) and bool((pad_u[m:] == -1).all())
    assert torch.equal(pad_o[:m], want_o) and bool((pad_o[m:] == 0).all())
    # comm.coalesce_rows: num_rows and scale change nothing off the GPU
    uniq2, out2 = coalesce_rows(ids, vals, num_rows=rows, scale=scale)
    assert torch.equal(uniq2, want_u) and torch.equal(out2, want_o)
