"""Microbenchmark: fused dropout + residual + LayerNorm (ext.ln_drop_fwd /
ln_drop_bwd, the mask regenerated from a counter hash) against the composite
the BERT layer ran before: F.dropout (dropped copy + bool mask), ln_fwd /
ln_bwd, and the mask multiply autograd adds in backward.

Shapes are [N, H] bf16 sublayer outputs: [4096, 768] (BERT-base, batch 32,
S 128), [4096, 1024] (BERT-large) and [16384, 768]. Forward and backward are
timed apart; the two paths alternate (device events around `--iters`
back-to-back calls, after warm-up) for `--rounds` rounds and the median round
is reported, with min..max, and the bytes each path needs over its time.
Needs a GPU:
    python tools/ln_dropout_microbench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(4096, 768), (4096, 1024), (16384, 768)]
P = 0.1
# needed traffic in units of T = N * H * 2 bytes (docs/KERNELS.md, ln_ops):
# fused fwd reads x, res, writes y, u; fused bwd reads dy, u, writes dx,
# dres. Composite fwd: dropout reads x, writes copy + 1-byte mask, ln_fwd
# reads copy, res, writes y, u; bwd: ln_bwd_dx reads dy, u, writes dx,
# ln_bwd_gb reads dy, u, the mask multiply reads dx + mask, writes dx'.
T_UNITS = {"fused_fwd": 4.0, "comp_fwd": 6.5, "fused_bwd": 4.0,
           "comp_bwd": 7.5}


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
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ln_dropout_microbench needs a GPU")
    from autodist_amd.ops import api as ops_api
    assert ops_api.has_gpu_ops()
    ext = ops_api.ext()
    dev = torch.device("cuda")
    results = []
    print(f"{'shape':>12} {'pass':>4} {'fused us':>9} {'comp us':>9} "
          f"{'speedup':>8} {'fused GB/s':>11} {'comp GB/s':>10}")
    for N, H in SHAPES:
        gen = torch.Generator(device=dev).manual_seed(N + H)
        x = torch.randn(N, H, generator=gen, device=dev).bfloat16()
        res = torch.randn(N, H, generator=gen, device=dev).bfloat16()
        dy = torch.randn(N, H, generator=gen, device=dev).bfloat16()
        gamma = torch.rand(H, generator=gen, device=dev) + 0.5
        beta = torch.randn(H, generator=gen, device=dev)
        eps, seed = 1e-12, 12345
        _, u, mean, rstd = ext.ln_drop_fwd(x, res, gamma, beta, eps, P, seed)
        mask = torch.rand(N, H, generator=gen, device=dev) >= P
        scale = 1.0 / (1.0 - P)

        def fused_fwd():
            ext.ln_drop_fwd(x, res, gamma, beta, eps, P, seed)

        def comp_fwd():
            # what nn.Dropout runs in training: copy + bool mask, then LN
            xd, _ = torch.native_dropout(x, P, True)
            ext.ln_fwd(xd, res, gamma, beta, eps)

        def fused_bwd():
            ext.ln_drop_bwd(dy, u, gamma, mean, rstd, P, seed)

        def comp_bwd():
            dx, _, _ = ext.ln_bwd(dy, u, gamma, mean, rstd)
            torch.ops.aten.native_dropout_backward(dx, mask, scale)

        pairs = {"fwd": (fused_fwd, comp_fwd), "bwd": (fused_bwd, comp_bwd)}
        for name, (fused, comp) in pairs.items():
            for _ in range(args.warmup):
                fused()
                comp()
            torch.cuda.synchronize()
            t_f, t_c = [], []
            for _ in range(args.rounds):
                t_f.append(_time(fused, args.iters))
                t_c.append(_time(comp, args.iters))
            f_us, c_us = statistics.median(t_f), statistics.median(t_c)
            t_bytes = N * H * 2
            f_b = T_UNITS[f"fused_{name}"] * t_bytes
            c_b = T_UNITS[f"comp_{name}"] * t_bytes
            rec = {"N": N, "H": H, "pass": name, "p": P,
                   "fused_us": round(f_us, 2), "comp_us": round(c_us, 2),
                   "fused_us_rounds": [round(v, 2) for v in t_f],
                   "comp_us_rounds": [round(v, 2) for v in t_c],
                   "speedup": round(c_us / f_us, 3),
                   "fused_bytes": int(f_b), "comp_bytes": int(c_b),
                   "fused_gbps": round(f_b / f_us / 1e3, 1),
                   "comp_gbps": round(c_b / c_us / 1e3, 1)}
            results.append(rec)
            print(f"{f'{N}x{H}':>12} {name:>4} {f_us:>9.2f} {c_us:>9.2f} "
                  f"{c_us / f_us:>7.2f}x {rec['fused_gbps']:>11.1f} "
                  f"{rec['comp_gbps']:>10.1f}", flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
