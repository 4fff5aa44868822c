"""Microbenchmark of the fused BN kernels at the BN layers of ResNet-50.

    python tools/bn_microbench.py [--batch 512] [--miopen] [--iters 20]

Runs on a GPU. For every distinct BN layer of ResNet-50 (channels, spatial
size, kind: relu / add+relu / plain, and how many such layers the network
has) it times one forward+backward through fused_bn_train and reports the
device time of each kernel family separately -- forward reduce, forward
finalize, forward apply, backward reduce, backward finalize, backward apply --
taken from torch.profiler's kernel records. The last table weights the layers
by their count: per-step time, bytes moved (computed from the shapes) and the
achieved rate of every family, so a change to one kernel can be judged
without the full model. --miopen adds the wall-clock comparison against
MIOpen BN + add + relu.

Each layer rotates through enough input sets to exceed the 256 MiB Infinity
Cache; one set timed in a loop would be read from cache, not from HBM.
"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (C, H = W, kind, layers of this kind in ResNet-50 v1.5): 53 in all,
# 11.11 M elements per image
LAYERS = [
    (64, 112, "relu", 1),
    (64, 56, "relu", 6), (256, 56, "add", 3), (256, 56, "plain", 1),
    (128, 56, "relu", 1), (128, 28, "relu", 7), (512, 28, "add", 4),
    (512, 28, "plain", 1),
    (256, 28, "relu", 1), (256, 14, "relu", 11), (1024, 14, "add", 6),
    (1024, 14, "plain", 1),
    (512, 14, "relu", 1), (512, 7, "relu", 5), (2048, 7, "add", 3),
    (2048, 7, "plain", 1),
]
assert sum(n for *_, n in LAYERS) == 53

FAMILIES = ["bn_fwd_reduce", "bn_fwd_finalize", "bn_fwd_apply",
            "bn_bwd_reduce", "bn_bwd_finalize", "bn_bwd_apply"]
ROTATE_BYTES = 1 << 30


def family_bytes(kind, n_elem, C, gm_rows, has_mask):
    """Bytes each kernel family has to move for one bf16 layer, from shapes.
    With the packed mask, backward reads 1 bit where it read a bf16 y."""
    e = 2 * n_elem                      # one bf16 pass over the tensor
    mask = n_elem // 8 if (has_mask and kind != "plain") else 0
    # what backward reads for y > 0: nothing, the mask, or y itself
    sign = 0 if kind == "plain" else (mask if has_mask else e)
    part = 2 * gm_rows * C * 4          # the two fp32 partial matrices
    return {
        "bn_fwd_reduce": e + part,
        "bn_fwd_finalize": part,
        "bn_fwd_apply": e * (3 if kind == "add" else 2) + mask,
        "bn_bwd_reduce": 2 * e + sign + part,
        "bn_bwd_finalize": part,
        "bn_bwd_apply": e * (4 if kind == "add" else 3) + sign,
    }


def reduce_gm(M, C):
    """Partial rows of the two-stage reductions (bn_reduce_gm in ext.hip)."""
    tx = min(C // 8, 256)
    rows = -(-M // (256 // tx))
    return min(max(-(-rows // 32), 64), 512, rows)


def time_fn(fn, iters, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3


def kernel_times(fn, iters):
    """us per call of every BN kernel family over `iters` calls of fn."""
    from torch.profiler import ProfilerActivity, profile
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    out = dict.fromkeys(FAMILIES, 0.0)
    seen = dict.fromkeys(FAMILIES, 0)
    for ev in prof.key_averages():
        for fam in FAMILIES:
            if fam + "_kernel" in ev.key:
                t = getattr(ev, "device_time_total", None)
                if t is None:
                    t = ev.cuda_time_total
                out[fam] += t / iters
                seen[fam] += ev.count
    missing = [f for f in FAMILIES if seen[f] != iters]
    if missing:
        raise RuntimeError(f"profiler recorded {seen}, expected {iters} "
                           f"launches of each BN kernel")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512,
                    help="per-GPU batch (bench.py runs ResNet-50 at 512)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--miopen", action="store_true",
                    help="also time MIOpen BN + add + relu (wall clock)")
    args = ap.parse_args()

    from autodist_amd.ops import api
    from autodist_amd.ops.fused_bn import fused_bn_train
    has_mask = hasattr(api.ext(), "bn_fwd_train_mask")
    dev = torch.device("cuda")
    N = args.batch
    print(f"# batch {N}, bf16, packed ReLU mask: {has_mask}; us per call")
    print(f"{'C':>5} {'HW':>4} {'kind':>5} {'x':>3} "
          + " ".join(f"{f[3:]:>13}" for f in FAMILIES)
          + (f" {'fusedFB':>9} {'miopenFB':>9}" if args.miopen else ""))
    step_us = dict.fromkeys(FAMILIES, 0.0)
    step_bytes = dict.fromkeys(FAMILIES, 0)
    for (C, HW, kind, count) in LAYERS:
        n_elem = N * C * HW * HW
        sets = max(2, min(16, ROTATE_BYTES // (2 * n_elem)))
        mk = lambda: torch.randn(N, C, HW, HW, device=dev,  # noqa: E731
                                 dtype=torch.bfloat16).contiguous(
                                     memory_format=torch.channels_last)
        xs = [mk() for _ in range(sets)]
        rs = [mk() for _ in range(sets)] if kind == "add" else None
        gs = [mk() for _ in range(sets)]
        w = torch.nn.Parameter(torch.rand(C, device=dev) + 0.5)
        b = torch.nn.Parameter(torch.randn(C, device=dev))
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        ws = (torch.empty(2 * 512 + 4, C, device=dev),
              torch.empty(2 * 512 + 3, C, device=dev))
        turn = [0]

        def fused_fwd_bwd():
            i = turn[0] = (turn[0] + 1) % sets
            xg = xs[i].detach().requires_grad_(True)
            rg = rs[i].detach().requires_grad_(True) if rs else None
            y = fused_bn_train(xg, w, b, rm, rv, relu=kind != "plain",
                               residual=rg, ws=ws)
            y.backward(gs[i])

        kt = kernel_times(fused_fwd_bwd, args.iters)
        fb = family_bytes(kind, n_elem, C, reduce_gm(N * HW * HW, C),
                          has_mask)
        for f in FAMILIES:
            step_us[f] += count * kt[f]
            step_bytes[f] += count * fb[f]
        line = (f"{C:5d} {HW:4d} {kind:>5} {count:3d} "
                + " ".join(f"{kt[f]:13.1f}" for f in FAMILIES))
        if args.miopen:
            bn = torch.nn.BatchNorm2d(C).to(dev)

            def miopen_fwd_bwd():
                i = turn[0] = (turn[0] + 1) % sets
                xg = xs[i].detach().requires_grad_(True)
                with torch.autocast("cuda", torch.bfloat16):
                    y = bn(xg)
                    if rs:
                        y = y + rs[i].detach().requires_grad_(True)
                    if kind != "plain":
                        y = torch.relu(y)
                y.backward(gs[i])

            line += (f" {time_fn(fused_fwd_bwd, args.iters) * 1e3:9.1f}"
                     f" {time_fn(miopen_fwd_bwd, args.iters) * 1e3:9.1f}")
        print(line, flush=True)
        del xs, rs, gs

    print(f"# per training step (53 layers, batch {N}), bytes from shapes")
    print(f"{'family':>16} {'ms/step':>9} {'GB/step':>9} {'TB/s':>7}")
    for f in FAMILIES:
        ms, gb = step_us[f] / 1e3, step_bytes[f] / 1e9
        print(f"{f:>16} {ms:9.3f} {gb:9.2f} {gb / ms:7.2f}")
    print(f"{'all BN kernels':>16} {sum(step_us.values()) / 1e3:9.3f} "
          f"{sum(step_bytes.values()) / 1e9:9.2f}")


if __name__ == "__main__":
    main()
