"""Shared by the sampled softmax tests: seeded inputs and the float64
reference, written out from the formulas (no autograd)."""
import math

import torch

from autodist_amd.ops.sampled_softmax import LogUniformSampler


def reference(h, w, b, t, c, lq_t, lq_s, g):
    """float64 loss rows, dH, per-row weight-gradient values over cat(c, t)
    and the dense db, plus the intermediates the loss bound needs."""
    h, w, g = h.double(), w.double(), g.double()
    b = torch.zeros(w.size(0), dtype=torch.float64) if b is None \
        else b.double()
    wg, wt = w[c], w[t]
    z0 = (h * wt).sum(1) + b[t] - lq_t.double()
    z = h @ wg.t() + b[c] - lq_s.double()
    z = z.masked_fill(c[None, :] == t[:, None], float("-inf"))
    lse = torch.logsumexp(torch.cat([z0[:, None], z], 1), 1)
    dz = (z - lse[:, None]).exp() * g[:, None]
    dz0 = ((z0 - lse).exp() - 1) * g
    vals = torch.cat([dz.t() @ h, dz0[:, None] * h])
    db = torch.zeros_like(b).index_add_(0, torch.cat([c, t]),
                                        torch.cat([dz.sum(0), dz0]))
    return {"loss": lse - z0, "dH": dz @ wg + dz0[:, None] * wt,
            "dW_rows": vals, "db": db, "dz": dz,
            "z": z, "z0": z0, "lse": lse}


def make_inputs(N, S, P, V, seed, hit_share=0.6):
    """Inputs with duplicate candidates; for `hit_share` of the rows the
    target is one of the candidates."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, P, generator=g)
    w = torch.randn(V, P, generator=g) * 0.3
    b = torch.randn(V, generator=g)
    c = torch.randint(0, V, (S,), generator=g)
    c[S // 2:S // 2 + S // 4] = c[:S // 4]
    t = torch.randint(0, V, (N,), generator=g)
    hits = math.ceil(hit_share * N)
    t[:hits] = c[torch.randint(0, S, (hits,), generator=g)]
    sampler = LogUniformSampler(V, S)
    return h, w, b, t, c, sampler.logq_true(t), sampler.logq_true(c)
