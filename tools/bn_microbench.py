"""Microbenchmark of the fused BN kernels at the BN layers of ResNet-50.

    python tools/bn_microbench.py [--batch 512] [--miopen] [--iters 20] [--ab]

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

Two kinds run more than one BN kernel chain: `pool` is the stem's
bn -> relu -> 3x3/2 max-pool (FusedBatchNorm2d.forward_pool) and `add_bn` the
tail of a block with a downsample, relu(bn3(z) + bn_ds(zd))
(forward_add_bn, two BN layers). --ab times these five layers a second time
through the split path they replace (bn -> F.max_pool2d; bn_ds, then bn3 with
a residual), in the same build, and prints both per kernel family; torch's
pool kernels and whatever else the split path launches (fills, copies) are
counted there.

--ab also times the `add` and `add_bn` tails with the block-output gradient
arriving as two addends, as it does inside the network ("join"): once through
the two-handle tails (forward_add_pair / forward_add_bn_pair: the add happens
in bn_bwd_reduce_join, the apply reads its dz; the add_bn tail runs both of
its BNs through bn_bwd_reduce_join2 and bn_bwd_apply2) and once through the
single-handle tails, where autograd adds the two gradients with a stand-alone
kernel first and backward is bn_bwd_mask (with dres for `add`). The last
table weights these by the 15 block boundaries of ResNet-50 that have two
consumers (every tail but layer4's last).

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
    (64, 112, "pool", 1),
    (64, 56, "relu", 6), (256, 56, "add", 2), (256, 56, "add_bn", 1),
    (128, 56, "relu", 1), (128, 28, "relu", 7), (512, 28, "add", 3),
    (512, 28, "add_bn", 1),
    (256, 28, "relu", 1), (256, 14, "relu", 11), (1024, 14, "add", 5),
    (1024, 14, "add_bn", 1),
    (512, 14, "relu", 1), (512, 7, "relu", 5), (2048, 7, "add", 2),
    (2048, 7, "add_bn", 1),
]
BN_PER_KIND = {"relu": 1, "add": 1, "plain": 1, "pool": 1, "add_bn": 2}
assert sum(n * BN_PER_KIND[k] for _, _, k, n in LAYERS) == 53

# torch's bf16 add, as autograd launches it to sum two gradients (the fp32
# adds that accumulate parameter gradients stay in "other")
BF16_ADD = "CUDAFunctor_add<c10::BFloat16>"
# kernel families: our kernels by their name without "_kernel", torch's pool
# kernels by theirs; "other" is every other kernel the timed call launched
FAMILIES = ["bn_fwd_reduce", "bn_fwd_finalize", "bn_fwd_apply",
            "bn_fwd_pool_apply", "bn_fwd_apply_add_bn",
            "max_pool_forward_nhwc",
            "bn_bwd_reduce", "bn_bwd_reduce_join", "bn_bwd_reduce_join2",
            "bn_bwd_finalize", "bn_bwd_apply", "bn_bwd_apply2",
            "max_pool_backward_nhwc", BF16_ADD, "other"]
ROTATE_BYTES = 1 << 30


def _bn_bytes(kind, n_elem, C, gm_rows, has_mask):
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


def family_bytes(kind, n_elem, C, gm_rows, has_mask, split=False):
    """Bytes each kernel family has to move for one bf16 layer, from shapes
    (n_elem: elements of the BN input). With the packed mask, backward reads
    1 bit where it read a bf16 y. `other` kernels are not given bytes."""
    out = dict.fromkeys(FAMILIES, 0)
    e = 2 * n_elem
    part = 2 * gm_rows * C * 4
    if kind == "pool" and split:
        out.update(_bn_bytes("relu", n_elem, C, gm_rows, has_mask))
        # pooled y is a quarter; torch keeps int64 indices, 8 B per pooled
        # element = one bf16 pass of the full tensor
        out["max_pool_forward_nhwc"] = e + e // 4 + e
        out["max_pool_backward_nhwc"] = e // 4 + e + e
    elif kind == "pool":
        words = n_elem // 8             # 4 B per 8 pooled channels
        out.update({
            "bn_fwd_reduce": e + part, "bn_fwd_finalize": part,
            "bn_fwd_pool_apply": e + e // 4 + words,
            "bn_bwd_reduce": e + e // 4 + words + part,
            "bn_bwd_finalize": part,
            "bn_bwd_apply": e + e // 4 + words + e,
        })
    elif kind == "add_bn" and split:
        a = _bn_bytes("add", n_elem, C, gm_rows, has_mask)
        b = _bn_bytes("plain", n_elem, C, gm_rows, has_mask)
        out.update({f: a[f] + b[f] for f in a})
    elif kind == "add_bn":
        mask = n_elem // 8
        out.update({
            "bn_fwd_reduce": 2 * (e + part), "bn_fwd_finalize": 2 * part,
            "bn_fwd_apply_add_bn": 3 * e + mask,
            "bn_bwd_reduce": 2 * (2 * e + mask + part),
            "bn_bwd_finalize": 2 * part,
            "bn_bwd_apply": 2 * (3 * e + mask),
        })
    else:
        out.update(_bn_bytes(kind, n_elem, C, gm_rows, has_mask))
    return out


def expected_launches(kind, split):
    """Launches of each of our families (and torch's pool kernels) in one
    forward+backward of a layer; `other` is not checked."""
    n = dict.fromkeys(FAMILIES, 0)
    two = 2 if kind == "add_bn" else 1
    for f in ("bn_fwd_reduce", "bn_fwd_finalize", "bn_bwd_reduce",
              "bn_bwd_finalize", "bn_bwd_apply"):
        n[f] = two
    if kind == "pool" and not split:
        n["bn_fwd_pool_apply"] = 1
    elif kind == "add_bn" and not split:
        n["bn_fwd_apply_add_bn"] = 1
    else:
        n["bn_fwd_apply"] = two
        if kind == "pool":
            n["max_pool_forward_nhwc"] = n["max_pool_backward_nhwc"] = 1
    return n


def join_bytes(kind, n_elem, C, gm_rows, pair):
    """family_bytes for a tail whose dy arrives as two addends. pair: the
    join reduce reads x and both addends and writes dz, the apply reads x and
    dz; for add_bn one reduce reads z, zd and both addends and writes dz (and
    three partial matrices, not two), and one apply reads z, zd and dz and
    writes both dx. Otherwise torch's add (two reads, one write) comes first
    and backward is the single-gradient one, which reads the mask in reduce
    and apply and, for `add`, writes dres."""
    e, mask, part = 2 * n_elem, n_elem // 8, 2 * gm_rows * C * 4
    out = family_bytes(kind, n_elem, C, gm_rows, True)
    if not pair:
        out[BF16_ADD] = 3 * e
        return out
    out["bn_bwd_reduce"] = out["bn_bwd_apply"] = 0
    if kind == "add_bn":
        out["bn_bwd_reduce_join2"] = 5 * e + mask + part * 3 // 2
        out["bn_bwd_apply2"] = 5 * e
    else:
        out["bn_bwd_reduce_join"] = 4 * e + mask + part
        out["bn_bwd_apply"] = 3 * e
    return out


def join_launches(kind, pair):
    n = expected_launches(kind, False)
    if pair and kind == "add_bn":
        n["bn_bwd_reduce_join2"] = n["bn_bwd_apply2"] = 1
        n["bn_bwd_reduce"] = n["bn_bwd_apply"] = 0
    elif pair:
        n["bn_bwd_reduce_join"] = 1
        n["bn_bwd_reduce"] -= 1
    else:
        n[BF16_ADD] = 1
    return n


# tails of ResNet-50 whose output has two consumers: all but layer4's last
def join_count(C, kind, count):
    return count - 1 if (C, kind) == (2048, "add") else count


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


def kernel_times(fn, iters, expect):
    """us per call of every kernel family over `iters` calls of fn."""
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
        t = getattr(ev, "device_time_total", None)
        if t is None:
            t = ev.cuda_time_total
        if not t:
            continue
        fam = next((f for f in FAMILIES
                    if (f + "_kernel" if f.startswith("bn_") else f)
                    in ev.key), "other")
        out[fam] += t / iters
        seen[fam] += ev.count
    wrong = {f: seen[f] for f in FAMILIES
             if f != "other" and seen[f] != iters * expect[f]}
    if wrong:
        raise RuntimeError(f"profiler recorded {wrong}, expected {iters} x "
                           f"{expect}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512,
                    help="per-GPU batch (bench.py runs ResNet-50 at 512)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--miopen", action="store_true",
                    help="also time MIOpen BN + add + relu (wall clock)")
    ap.add_argument("--ab", action="store_true",
                    help="time the pool / add_bn layers through the split "
                         "path as well and print both")
    args = ap.parse_args()

    from autodist_amd.ops import api, fused_bn
    from autodist_amd.ops.fused_bn import FusedBatchNorm2d, fused_bn_train
    has_mask = hasattr(api.ext(), "bn_fwd_train_mask")
    dev = torch.device("cuda")
    N = args.batch
    print(f"# batch {N}, bf16, packed ReLU mask: {has_mask}; us per call")
    print(f"{'C':>5} {'HW':>4} {'kind':>5} {'x':>3} "
          + " ".join(f"{f[3:] if f.startswith('bn_') else f[:13]:>13}"
                     for f in FAMILIES)
          + (f" {'fusedFB':>9} {'miopenFB':>9}" if args.miopen else ""))
    step_us = dict.fromkeys(FAMILIES, 0.0)
    step_bytes = dict.fromkeys(FAMILIES, 0)
    # the pool / add_bn layers, fused and (--ab) split: kind -> path -> sums
    ab_us = {k: {p: dict.fromkeys(FAMILIES, 0.0) for p in ("fused", "split")}
             for k in ("pool", "add_bn")}
    ab_bytes = {k: {p: dict.fromkeys(FAMILIES, 0) for p in ("fused", "split")}
                for k in ("pool", "add_bn")}
    join_us = {p: dict.fromkeys(FAMILIES, 0.0) for p in ("fused", "split")}
    join_bytes_sum = {p: dict.fromkeys(FAMILIES, 0)
                      for p in ("fused", "split")}
    for (C, HW, kind, count) in LAYERS:
        n_elem = N * C * HW * HW
        sets = max(2, min(16, ROTATE_BYTES // (2 * n_elem)))
        mk = lambda hw=HW: torch.randn(N, C, hw, hw, device=dev,  # noqa: E731
                                       dtype=torch.bfloat16).contiguous(
                                           memory_format=torch.channels_last)
        xs = [mk() for _ in range(sets)]
        rs = [mk() for _ in range(sets)] if kind in ("add", "add_bn") else None
        gs = [mk((HW - 1) // 2 + 1 if kind == "pool" else HW)
              for _ in range(sets)]
        w = torch.nn.Parameter(torch.rand(C, device=dev) + 0.5)
        b = torch.nn.Parameter(torch.randn(C, device=dev))
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        ws = (torch.empty(2 * 512 + 4, C, device=dev),
              torch.empty(2 * 512 + 3, C, device=dev))
        turn = [0]

        bn = FusedBatchNorm2d(C, relu=True).to(dev).train()
        bn_d = FusedBatchNorm2d(C, relu=False).to(dev).train()

        def fused_fwd_bwd():
            i = turn[0] = (turn[0] + 1) % sets
            xg = xs[i].detach().requires_grad_(True)
            rg = rs[i].detach().requires_grad_(True) if rs else None
            if kind == "pool":
                y = bn.forward_pool(xg)
            elif kind == "add_bn":
                y = bn.forward_add_bn(xg, rg, bn_d)
            else:
                y = fused_bn_train(xg, w, b, rm, rv, relu=kind != "plain",
                                   residual=rg, ws=ws)
            y.backward(gs[i])

        gm = reduce_gm(N * HW * HW, C)
        kt = kernel_times(fused_fwd_bwd, args.iters,
                          expected_launches(kind, False))
        fb = family_bytes(kind, n_elem, C, gm, has_mask)
        for f in FAMILIES:
            step_us[f] += count * kt[f]
            step_bytes[f] += count * fb[f]
        if kind in ab_us:
            paths = [("fused", kt, fb)]
            if args.ab:
                fused_bn.SPLIT_PATH = True
                try:
                    paths.append(("split", kernel_times(
                        fused_fwd_bwd, args.iters,
                        expected_launches(kind, True)),
                        family_bytes(kind, n_elem, C, gm, has_mask, True)))
                finally:
                    fused_bn.SPLIT_PATH = False
            for path, t, nb in paths:
                for f in FAMILIES:
                    ab_us[kind][path][f] += count * t[f]
                    ab_bytes[kind][path][f] += count * nb[f]
        line = (f"{C:5d} {HW:4d} {kind:>5} {count:3d} "
                + " ".join(f"{kt[f]:13.1f}" for f in FAMILIES))
        join_lines = []
        if args.ab and kind in ("add", "add_bn"):
            g2 = [mk() for _ in range(sets)]

            def join_fwd_bwd(pair):
                i = turn[0] = (turn[0] + 1) % sets
                xg = xs[i].detach().requires_grad_(True)
                rg = rs[i].detach().requires_grad_(True)
                if kind == "add_bn":
                    y = bn.forward_add_bn(xg, rg, bn_d, pair=pair)
                else:
                    y = fused_bn_train(xg, w, b, rm, rv, relu=True,
                                       residual=rg, ws=ws, pair=pair)
                # one handle fed both gradients: autograd adds them first
                torch.autograd.backward(y if pair else [y, y], [gs[i], g2[i]])

            for path, pair in (("fused", True), ("split", False)):
                t = kernel_times(lambda: join_fwd_bwd(pair), args.iters,
                                 join_launches(kind, pair))
                nb = join_bytes(kind, n_elem, C, gm, pair)
                for f in FAMILIES:
                    join_us[path][f] += join_count(C, kind, count) * t[f]
                    join_bytes_sum[path][f] += \
                        join_count(C, kind, count) * nb[f]
                join_lines.append(
                    f"{'':5} {'':4} {'join':>5} {path[:3]:>3} "
                    + " ".join(f"{t[f]:13.1f}" for f in FAMILIES))
            del g2
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
        for jl in join_lines:
            print(jl, flush=True)
        del xs, rs, gs

    print(f"# per training step (53 layers, batch {N}), bytes from shapes")
    print(f"{'family':>24} {'ms/step':>9} {'GB/step':>9} {'TB/s':>7}")
    for f in FAMILIES:
        ms, gb = step_us[f] / 1e3, step_bytes[f] / 1e9
        rate = f"{gb / ms:7.2f}" if ms and gb else f"{'-':>7}"
        print(f"{f:>24} {ms:9.3f} {gb:9.2f} {rate}")
    print(f"{'all kernels above':>24} {sum(step_us.values()) / 1e3:9.3f} "
          f"{sum(step_bytes.values()) / 1e9:9.2f}")
    if not args.ab:
        return
    for kind, what in (("pool", "the stem layer"),
                       ("add_bn", "the four downsample tails")):
        print(f"# {kind}: {what}, per training step, split path | fused")
        print(f"{'family':>24} {'ms':>8} {'GB':>7} {'TB/s':>6} | "
              f"{'ms':>8} {'GB':>7} {'TB/s':>6}")
        for f in FAMILIES:
            cells = []
            for path in ("split", "fused"):
                ms = ab_us[kind][path][f] / 1e3
                gb = ab_bytes[kind][path][f] / 1e9
                rate = f"{gb / ms:6.2f}" if ms and gb else f"{'-':>6}"
                cells.append(f"{ms:8.3f} {gb:7.2f} {rate}")
            print(f"{f:>24} " + " | ".join(cells))
        tot = [sum(ab_us[kind][p].values()) / 1e3 for p in ("split", "fused")]
        gbs = [sum(ab_bytes[kind][p].values()) / 1e9
               for p in ("split", "fused")]
        print(f"{'sum':>24} {tot[0]:8.3f} {gbs[0]:7.2f} {'':>6} | "
              f"{tot[1]:8.3f} {gbs[1]:7.2f}")
    print("# join: the 15 two-consumer block boundaries (11 add, 4 add_bn "
          "tails), forward + backward per training step, autograd's add + "
          "single-gradient backward | two-handle tails")
    print(f"{'family':>24} {'ms':>8} {'GB':>7} {'TB/s':>6} | "
          f"{'ms':>8} {'GB':>7} {'TB/s':>6}")
    for f in FAMILIES:
        cells = []
        for path in ("split", "fused"):
            ms = join_us[path][f] / 1e3
            gb = join_bytes_sum[path][f] / 1e9
            rate = f"{gb / ms:6.2f}" if ms and gb else f"{'-':>6}"
            cells.append(f"{ms:8.3f} {gb:7.2f} {rate}")
        print(f"{f:>24} " + " | ".join(cells))
    tot = [sum(join_us[p].values()) / 1e3 for p in ("split", "fused")]
    gbs = [sum(join_bytes_sum[p].values()) / 1e9 for p in ("split", "fused")]
    print(f"{'sum':>24} {tot[0]:8.3f} {gbs[0]:7.2f} {'':>6} | "
          f"{tot[1]:8.3f} {gbs[1]:7.2f}")
    bwd = ("bn_bwd_reduce", "bn_bwd_reduce_join", "bn_bwd_reduce_join2",
           "bn_bwd_apply", "bn_bwd_apply2", BF16_ADD)
    tb = [sum(join_us[p][f] for f in bwd) / 1e3 for p in ("split", "fused")]
    print(f"{'backward streams only':>24} {tb[0]:8.3f} {'':>14} | {tb[1]:8.3f}")


if __name__ == "__main__":
    main()
