"""Microbenchmark: the sort-free deterministic coalesce (coalesce_rows_ranked,
ops/csrc/sparse_ops.hip) vs the sorting one it replaces on the sparse sync
path (segment_coalesce: at::_unique + zeros + float-atomic scatter-add), at
the NCF and LM1B embedding shapes.

Each case first checks that the two paths agree within fp32 summation-order
noise, then times them alternately (device events around `--iters`
back-to-back calls, after warm-up), `--rounds` times, and reports the median
round and the min..max spread. `ranked` is the exact mode (one host read, as
the sorting path has); `ranked nosync` is exact=False. Needs a GPU:
    python tools/coalesce_microbench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (label, table rows, row width D, ids per step, id distribution)
CASES = [
    ("ncf item mf", 26744, 64, 4096, "uniform"),
    ("ncf item mlp", 26744, 128, 4096, "uniform"),
    ("ncf user mf", 138493, 64, 4096, "uniform"),
    ("ncf user mlp", 138493, 128, 4096, "uniform"),
    ("ncf item mf zipf", 26744, 64, 4096, "zipf"),
    ("lm1b embedding", 793470, 512, 128 * 20, "zipf"),
]


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
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("coalesce_microbench needs a GPU")
    from autodist_amd.ops import api as ops_api
    assert ops_api.has_gpu_ops()
    gen = torch.Generator().manual_seed(0)
    results = []
    print(f"{'case':>18} {'rows':>7} {'D':>4} {'n':>5} {'uniq':>5} "
          f"{'sort us':>16} {'ranked us':>16} {'nosync us':>16}")
    for label, rows, dim, n, dist in CASES:
        if dist == "zipf":
            ids = (rows ** torch.rand(n, generator=gen) - 1).long()
        else:
            ids = torch.randint(0, rows, (n,), generator=gen)
        ids = ids.cuda()
        vals = torch.randn(n, dim, generator=gen).cuda()
        paths = {
            "sort": lambda: ops_api.segment_coalesce(ids, vals),
            "ranked": lambda: ops_api.coalesce_rows_ranked(ids, vals, rows),
            "nosync": lambda: ops_api.coalesce_rows_ranked(
                ids, vals, rows, exact=False),
        }
        u_old, o_old = paths["sort"]()
        u_new, o_new = paths["ranked"]()
        assert torch.equal(u_old, u_new)
        # |values| ~ 1, at most a few hundred addends per row
        err = (o_old - o_new).abs().max().item()
        assert err <= 1e-3, err
        for fn in paths.values():
            for _ in range(args.warmup):
                fn()
        times = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, fn in paths.items():
                times[k].append(_time(fn, args.iters))
        row = {"case": label, "rows": rows, "dim": dim, "n": n,
               "uniq": int(u_new.shape[0]), "max_abs_diff": err}
        cols = []
        for k, t in times.items():
            row[k + "_us"] = statistics.median(t)
            row[k + "_us_min"], row[k + "_us_max"] = min(t), max(t)
            cols.append(f"{statistics.median(t):6.1f} "
                        f"({min(t):4.0f}..{max(t):4.0f})")
        print(f"{label:>18} {rows:7d} {dim:4d} {n:5d} {row['uniq']:5d} "
              + " ".join(f"{c:>16}" for c in cols), flush=True)
        results.append(row)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
