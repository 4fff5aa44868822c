"""Fused masked-LM head loss (lce_* kernels) against the torch composite:
forward + backward time from device events and peak memory of one call, at
the BERT-base benchmark shape, for two labelled fractions, with max_rows
unset and set to the labelled count rounded up to 64. The sides alternate in
one process (composite, kernels, kernels + max_rows, composite again).

Run: python tools/linear_ce_microbench.py [--log FILE]"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from autodist_amd.ops.fused_linear_ce import fused_linear_cross_entropy  # noqa

N, K, V = 4096, 768, 30522


def step(h, w, b, labels, max_rows):
    h.grad = w.grad = b.grad = None
    with torch.autocast("cuda", dtype=torch.bfloat16):
        loss = fused_linear_cross_entropy(h, w, b, labels, max_rows=max_rows)
    loss.backward()
    return loss


def timed(fn, rounds=3, iters=20):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(True), torch.cuda.Event(True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / iters)
    return min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    log = open(args.log, "w") if args.log else None
    torch.manual_seed(0)
    h = torch.randn(N, K, device="cuda", dtype=torch.bfloat16,
                    requires_grad=True)
    w = (torch.randn(V, K, device="cuda") * 0.02).requires_grad_(True)
    b = torch.zeros(V, device="cuda", requires_grad=True)
    for frac in (0.5, 0.15):
        labels = torch.randint(0, V, (N,), device="cuda")
        labels[torch.rand(N, device="cuda") >= frac] = -100
        cnt = int((labels != -100).sum())
        cap = -(-cnt // 64) * 64
        for name, env, mr in (("composite", "torch", None),
                              ("kernels", "", None),
                              (f"kernels max_rows={cap}", "", cap),
                              ("composite again", "torch", None)):
            os.environ["AUTODIST_LINEAR_CE"] = env
            lo, hi = timed(lambda: step(h, w, b, labels, mr))
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            loss = step(h, w, b, labels, mr)
            torch.cuda.synchronize()
            peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            line = (f"labelled {cnt}/{N} {name}: fwd+bwd {lo:.3f}..{hi:.3f} "
                    f"ms, peak above resident {peak:.0f} MiB, loss "
                    f"{loss.item():.5f}, |dW| {w.grad.norm().item():.5f}")
            print(line, flush=True)
            if log:
                print(line, file=log, flush=True)


if __name__ == "__main__":
    main()
