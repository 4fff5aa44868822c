"""Shared by the linear + cross-entropy tests: seeded inputs and the float64
reference, written out from the formulas (no autograd)."""
import torch


def make_inputs(N, V, K, labelled, seed):
    """bf16-representable h, W, b; `labelled` of the N labels are classes,
    the others -100, among them rows 0 and N - 1; one target is V - 1."""
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(N, K, generator=g).bfloat16().float()
    w = (torch.randn(V, K, generator=g) * 0.3).bfloat16().float()
    b = torch.randn(V, generator=g).bfloat16().float()
    labels = torch.randint(0, V, (N,), generator=g)
    inner = 1 + torch.randperm(N - 2, generator=g)
    labels[inner[labelled:]] = -100
    labels[0] = labels[N - 1] = -100
    labels[inner[0]] = V - 1
    return h, w, b, labels


def reference(h, w, b, labels, g):
    """float64 loss rows (0 where ignored), dh, dW, db for the loss
    sum(loss * g), and the logits, lse and target logits the bound needs."""
    h, w, g = h.double(), w.double(), g.double()
    b = torch.zeros(w.size(0), dtype=torch.float64) if b is None \
        else b.double()
    keep = labels != -100
    t = labels.clamp(min=0)
    z = h @ w.t() + b
    lse = torch.logsumexp(z, 1)
    zt = z.gather(1, t[:, None])[:, 0]
    dz = (z - lse[:, None]).exp()
    dz[torch.arange(len(t)), t] -= 1
    dz = dz * (g * keep)[:, None]
    return {"loss": (lse - zt) * keep, "dh": dz @ w, "dW": dz.t() @ h,
            "db": dz.sum(0), "z": z, "lse": lse, "zt": zt}
