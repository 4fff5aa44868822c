"""Microbenchmark of the sampled softmax loss on one GPU, two measurements:

1. op: sampled_softmax_loss through the ssm_* HIP kernels
   (ops/csrc/ssm_ops.hip) against the torch composite of the same build
   (AUTODIST_SAMPLED_SOFTMAX=torch) at N = 2560, P = 512, S = 8192 on an fp32
   table of 793,470 rows, under bf16 autocast with a sparse weight gradient;
   forward alone and forward + backward.
2. step: one training step (forward, backward, Adagrad through the engine)
   of the non-sharded lm1b_full(sparse=True) at batch 128 x 20 with
   num_sampled = 8192 against num_sampled = 0 (full softmax).

The two sides alternate in one process, `--rounds` times `--iters` calls
between device events after warm-up; the median round and the min..max
spread are reported. Needs a GPU:
    python tools/sampled_softmax_microbench.py [--only op|step] [--json f]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, P, S, V = 2560, 512, 8192, 793470
B, T = 128, 20


def _time(fn, iters):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # milliseconds per call


def _rounds(ts):
    return {"median_ms": round(statistics.median(ts), 4),
            "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


def _alternate(sides, args):
    """{name: callable} -> {name: round statistics}, sides interleaved."""
    for _ in range(args.warmup):
        for fn in sides.values():
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name in sides}
    for _ in range(args.rounds):
        for name, fn in sides.items():
            ts[name].append(_time(fn, args.iters))
    return {name: _rounds(v) for name, v in ts.items()}


def bench_op(args):
    from autodist_amd.ops.sampled_softmax import (LogUniformSampler,
                                                  sampled_softmax_loss)
    torch.manual_seed(0)
    h = torch.randn(N, P, device="cuda", requires_grad=True)
    w = (torch.randn(V, P, device="cuda") * 0.02).requires_grad_(True)
    b = torch.zeros(V, device="cuda", requires_grad=True)
    t = torch.randint(0, V, (N,), device="cuda")
    sampler = LogUniformSampler(V, S, seed=0)
    c, lq_s = sampler.sample("cuda")
    lq_t = sampler.logq_true(t)

    def call(path, backward):
        os.environ["AUTODIST_SAMPLED_SOFTMAX"] = path
        h.grad = w.grad = b.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = sampled_softmax_loss(h, w, b, t, c, lq_t, lq_s,
                                        sparse_grad=True)
        if backward:
            loss.backward()
        return loss

    l_k, l_t = call("hip", False).item(), call("torch", False).item()
    print(f"loss kernels {l_k:.5f} composite {l_t:.5f}")
    assert abs(l_k - l_t) < 2e-2 * max(abs(l_t), 1.0), (l_k, l_t)
    rec = {"N": N, "P": P, "S": S, "V": V}
    for name, bwd in (("fwd", False), ("fwd_bwd", True)):
        r = _alternate({"kernels": lambda: call("hip", bwd),
                        "composite": lambda: call("torch", bwd)}, args)
        r["speedup"] = round(r["composite"]["median_ms"]
                             / r["kernels"]["median_ms"], 3)
        rec[name] = r
    os.environ.pop("AUTODIST_SAMPLED_SOFTMAX")
    return rec


def bench_step(args):
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.models.lm1b import lm1b_full
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.resource_spec import ResourceSpec
    from autodist_amd.strategy import PS
    device = torch.device("cuda", 0)
    tokens = torch.randint(0, V, (B, T), device=device)
    targets = torch.randint(0, V, (B, T), device=device)

    def make(num_sampled):
        torch.manual_seed(0)
        model = lm1b_full(sparse=True, num_sampled=num_sampled).to(device)
        g = GraphItem()
        g.extend_model(model)
        opt = torch.optim.Adagrad(model.parameters(), lr=0.01)
        g.extend_optimizer_info(opt)
        engine = DistributedEngine(g, PS().build(g, ResourceSpec()), rank=0,
                                   world_size=1, device=device).setup()

        def step():
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = model.loss(tokens, targets)
            loss.backward()
            opt.step()
            return loss
        return step, engine

    sampled, e1 = make(S)
    full, e2 = make(0)
    r = _alternate({"num_sampled_8192": sampled, "full_softmax": full}, args)
    r["speedup"] = round(r["full_softmax"]["median_ms"]
                         / r["num_sampled_8192"]["median_ms"], 3)
    for e in (e1, e2):
        e.drain()
        e.teardown()
    return {"B": B, "T": T, "V": V, "optimizer": "Adagrad", **r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["op", "step"], default="")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sampled_softmax_microbench needs a GPU")
    rec = {}
    if args.only != "step":
        rec["op"] = bench_op(args)
        print(json.dumps(rec["op"]), flush=True)
    if args.only != "op":
        rec["step"] = bench_step(args)
        print(json.dumps(rec["step"]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
