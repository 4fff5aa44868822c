"""Microbenchmark: optimizer apply that reads the bf16 wire shard directly
(ops.api.fused_apply_wire) vs what the sharded schedule would otherwise do,
cast_back_f32 of the shard followed by the fp32 kernel (ops.api.fused_apply).

Shard sizes are an eighth of a model's parameter count (world 8): 3.2M
elements (ResNet-50) and 13.7M elements (BERT-base). Both paths apply the
same updates to equal buffers and must agree BIT FOR BIT before anything is
timed. They are timed alternately (device events around `--iters`
back-to-back calls, after warm-up), `--rounds` times; the median round is
reported with the bytes each path needs over its time. Needs a GPU:
    python tools/shard_apply_microbench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, shard elements)
SHARDS = [("resnet50/8", 3_200_000), ("bert-base/8", 13_700_000)]
# optimizer -> (hyper, fp32 state tensors read+written)
OPTIMIZERS = {
    "AdamW": ({"lr": 1e-3, "betas": (0.9, 0.999), "eps": 1e-8,
               "weight_decay": 1e-2}, 2),
    "SGD": ({"lr": 0.05, "momentum": 0.9}, 1),
}


def _time(fn, iters):
    start, end = torch.cuda.Event(True), torch.cuda.Event(True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters * 1e3  # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("shard_apply_microbench needs a GPU")
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    assert ops_api.has_gpu_ops()
    dev = torch.device("cuda")
    results = []
    print(f"{'shard':>12} {'opt':>6} {'n':>9} {'wire us':>8} {'cast us':>8} "
          f"{'speedup':>8} {'wire GB/s':>10} {'cast GB/s':>10}")
    for label, n in SHARDS:
        for opt, (hyper, n_state) in OPTIMIZERS.items():
            gen = torch.Generator().manual_seed(n)
            p0 = torch.randn(n, generator=gen).to(dev)
            wire = (torch.randn(n, generator=gen) * 1e-2).to(
                torch.bfloat16).to(dev)
            params = [p0.clone(), p0.clone()]
            states = [apply_mod.make_state(opt, p, hyper) for p in params]
            staging = torch.empty(n, dtype=torch.float32, device=dev)

            def direct():
                assert ops_api.fused_apply_wire(opt, params[0], wire,
                                                states[0], hyper)

            def cast_then_apply():
                ops_api.cast_back_f32(wire, staging)
                assert ops_api.fused_apply(opt, params[1], staging,
                                           states[1], hyper)

            for _ in range(args.warmup):
                direct()
                cast_then_apply()
            torch.cuda.synchronize()
            # same updates on both sides: bit-identical or nothing is timed
            pairs = [(params[0], params[1])] + [
                (states[0][k], states[1][k]) for k in states[0]]
            for a, b in pairs:
                assert torch.equal(a.view(torch.int32), b.view(torch.int32)), \
                    f"{label} {opt}: paths are not bit-identical"
            t_wire, t_cast = [], []
            for _ in range(args.rounds):
                t_wire.append(_time(direct, args.iters))
                t_cast.append(_time(cast_then_apply, args.iters))
            w_us = statistics.median(t_wire)
            c_us = statistics.median(t_cast)
            # needed bytes per element: param + state read and written in
            # fp32, the gradient read once (2 B wire; the cast path reads the
            # wire, writes and re-reads the fp32 staging copy: 2 + 4 + 4)
            rw = 8 * (1 + n_state)
            wire_bytes, cast_bytes = n * (rw + 2), n * (rw + 10)
            rec = {"shard": label, "optimizer": opt, "n": n,
                   "wire_us": round(w_us, 2), "cast_us": round(c_us, 2),
                   "wire_us_rounds": [round(x, 2) for x in t_wire],
                   "cast_us_rounds": [round(x, 2) for x in t_cast],
                   "speedup": round(c_us / w_us, 3),
                   "wire_bytes": wire_bytes, "cast_bytes": cast_bytes,
                   "wire_gbps": round(wire_bytes / w_us / 1e3, 1),
                   "cast_gbps": round(cast_bytes / c_us / 1e3, 1)}
            results.append(rec)
            print(f"{label:>12} {opt:>6} {n:>9} {w_us:>8.2f} {c_us:>8.2f} "
                  f"{c_us / w_us:>7.2f}x {rec['wire_gbps']:>10.1f} "
                  f"{rec['cast_gbps']:>10.1f}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
