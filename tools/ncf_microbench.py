"""Microbenchmark of the NeuMF model on one GPU: the fused HIP kernels
(ops/csrc/ncf_ops.hip) against the torch module path of the same build
(AUTODIST_NCF=torch) at B = 4096 on the MovieLens-20M tables (138,493 users,
26,744 items, mf_dim 64, MLP 256-128-64), fp32, sparse table gradients;
NeuMF.loss forward alone and forward + backward.

The two sides alternate in one process, `--rounds` times `--iters` calls
between device events after warm-up; the median round and the min..max
spread are reported. Needs a GPU:
    python tools/ncf_microbench.py [--batch B] [--json f]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ncf_microbench needs a GPU")
    from autodist_amd.models.ncf import ncf_movielens
    torch.manual_seed(0)
    model = ncf_movielens(sparse=True).cuda()
    B = args.batch
    users = torch.randint(0, 138493, (B,), device="cuda")
    items = torch.randint(0, 26744, (B,), device="cuda")
    labels = torch.randint(0, 2, (B,), device="cuda").float()

    def call(path, backward):
        os.environ["AUTODIST_NCF"] = path
        for p in model.parameters():
            p.grad = None
        loss = model.loss(users, items, labels)
        if backward:
            loss.backward()
        return loss

    l_k, l_t = call("fused", False).item(), call("torch", False).item()
    print(f"loss kernels {l_k:.6f} torch {l_t:.6f}")
    assert abs(l_k - l_t) < 1e-5 * max(abs(l_t), 1.0), (l_k, l_t)
    rec = {"B": B, "mf_dim": 64, "mlp_dims": [256, 128, 64]}
    for name, bwd in (("fwd", False), ("fwd_bwd", True)):
        r = _alternate({"kernels": lambda: call("fused", bwd),
                        "torch": lambda: call("torch", bwd)}, args)
        r["speedup"] = round(r["torch"]["median_ms"]
                             / r["kernels"]["median_ms"], 3)
        rec[name] = r
    os.environ.pop("AUTODIST_NCF")
    print(json.dumps(rec), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
