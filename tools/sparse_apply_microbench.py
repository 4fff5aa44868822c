"""Microbenchmark: fused row-wise optimizer apply (sparse_apply_rows_kernel)
vs the torch composite it replaces (index_select / addcmul_ / index_copy_ /
sqrt / index_add_), at the NCF and LM1B embedding shapes.

Both paths update the same tables with the same unique rows; they are timed
alternately (device events around `--iters` back-to-back calls, after
warm-up), `--rounds` times, and the median round is reported. At a few
thousand rows a call is launch-bound, so the GB/s column (needed bytes over
call time) is a per-call figure, not the kernel's bandwidth. Needs a GPU:
    python tools/sparse_apply_microbench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, table rows, row width D, ids per step, optimizer)
CASES = [
    ("ncf item mf", 26744, 64, 4096, "SGD"),
    ("ncf item mlp", 26744, 128, 4096, "SGD"),
    ("ncf user mf", 138493, 64, 4096, "SGD"),
    ("ncf user mlp", 138493, 128, 4096, "SGD"),
    ("ncf item mf", 26744, 64, 4096, "Adagrad"),
    ("ncf item mlp", 26744, 128, 4096, "Adagrad"),
    ("ncf user mf", 138493, 64, 4096, "Adagrad"),
    ("ncf user mlp", 138493, 128, 4096, "Adagrad"),
    ("lm1b embedding", 793470, 512, 128 * 20, "Adagrad"),
]
HYPER = {"SGD": {"lr": 0.05},
         "Adagrad": {"lr": 0.2, "lr_decay": 0.0, "eps": 1e-10}}


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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default="")
    ap.add_argument("--cases", default="",
                    help="only cases whose 'label optimizer' contains this")
    ap.add_argument("--path", choices=["both", "fused", "torch"],
                    default="both",
                    help="run one path only (for a kernel trace of its own; "
                         "--rounds x --iters timed calls after --warmup)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sparse_apply_microbench needs a GPU")
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel import apply as apply_mod
    assert ops_api.has_gpu_ops()
    dev = torch.device("cuda")
    results = []
    print(f"{'case':>16} {'opt':>8} {'rows':>7} {'D':>4} {'n':>5} "
          f"{'fused us':>9} {'torch us':>9} {'speedup':>8} {'GB/s(call)':>10}")
    for label, rows, dim, n_ids, opt in CASES:
        if args.cases not in f"{label} {opt}":
            continue
        gen = torch.Generator().manual_seed(rows + dim)
        # unique ids, as coalesce_rows hands them over (sorted)
        ids = torch.randperm(rows, generator=gen)[:n_ids].sort().values.to(dev)
        n = ids.numel()
        grads = (torch.rand(n, dim, generator=gen) * 2 - 1).to(dev)
        hyper = HYPER[opt]
        tables, states = [], []
        table0 = torch.rand(rows, dim, device=dev) * 2 - 1
        for _ in range(2):
            t = table0.clone()
            tables.append(t)
            states.append(apply_mod.make_state(opt, t, hyper))

        def fused():
            assert ops_api.fused_sparse_apply(opt, tables[0], ids, grads,
                                              states[0], hyper)

        def composite():
            apply_mod.apply_sparse_rows_torch(opt, tables[1], ids, grads,
                                              states[1], hyper)

        if args.path != "both":
            one = fused if args.path == "fused" else composite
            for _ in range(args.warmup):
                one()
            us = statistics.median(_time(one, args.iters)
                                   for _ in range(args.rounds))
            print(f"{label:>16} {opt:>8} {rows:>7} {dim:>4} {n:>5} "
                  f"{args.path} only: {us:.2f} us/call", flush=True)
            continue
        for _ in range(args.warmup):
            fused()
            composite()
        torch.cuda.synchronize()
        # same update on both sides: the outputs must agree
        err = (tables[0] - tables[1]).abs().max().item()
        assert err <= 1e-4, f"{label} {opt}: paths diverged ({err})"
        t_fused, t_torch = [], []
        for _ in range(args.rounds):
            t_fused.append(_time(fused, args.iters))
            t_torch.append(_time(composite, args.iters))
        f_us = statistics.median(t_fused)
        c_us = statistics.median(t_torch)
        # bytes the update needs: ids + grads read, param (+ state) rows
        # read and written
        state_tensors = 0 if opt == "SGD" else 1
        nbytes = n * 8 + n * dim * 4 * (1 + 2 * (1 + state_tensors))
        rec = {"case": label, "optimizer": opt, "rows": rows, "dim": dim,
               "n": n, "fused_us": round(f_us, 2), "torch_us": round(c_us, 2),
               "fused_us_rounds": [round(x, 2) for x in t_fused],
               "torch_us_rounds": [round(x, 2) for x in t_torch],
               "speedup": round(c_us / f_us, 2),
               "fused_call_gbps": round(nbytes / f_us / 1e3, 1),
               "max_abs_diff": err}
        results.append(rec)
        print(f"{label:>16} {opt:>8} {rows:>7} {dim:>4} {n:>5} {f_us:>9.2f} "
              f"{c_us:>9.2f} {c_us / f_us:>7.2f}x {rec['fused_call_gbps']:>10.1f}",
              flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
