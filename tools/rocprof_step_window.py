"""Per-step kernel table of a steady-state window of a rocprofv3 kernel trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \\
        python bench.py --gpus 1
    python tools/rocprof_step_window.py DIR/**/*kernel_trace.csv MARKER [STEPS]

MARKER is a substring of a kernel that runs exactly once per training step
(the stem's pool kernel: `bn_fwd_pool_apply` or `max_pool_forward_nhwc`). The
window runs from the STEPS-th last launch of that kernel (default 10) to the
last one, so it holds exactly STEPS steps of the replayed graph, after the
warm-up and any MIOpen find. Prints calls per step and ms per step of every BN
kernel instantiation, of the pool kernels and of torch's bf16 add (the
gradient adds at the block inputs), the BN-family totals, and the sum over
all kernels.
"""
import csv
import re
import sys

FAMILIES = ["bn_fwd_reduce", "bn_fwd_finalize", "bn_fwd_apply",
            "bn_fwd_pool_apply", "bn_fwd_apply_add_bn", "bn_bwd_reduce",
            "bn_bwd_reduce_join", "bn_bwd_reduce_join2", "bn_bwd_finalize",
            "bn_bwd_apply", "bn_bwd_apply2", "max_pool_forward_nhwc", "max_pool_backward_nhwc"]
# listed beside the BN kernels, not counted among them
ADD = "CUDAFunctor_add<c10::BFloat16>"


def short(name):
    """Kernel name with its template arguments, without the parameter list."""
    m = re.search(r"(bn_\w+_kernel(<[^>]*>)?|max_pool_\w+_nhwc)", name)
    if m is None and ADD in name:
        return ADD
    return m.group(1) if m else None


def main():
    path, marker = sys.argv[1], sys.argv[2]
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 10
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]),
                         r["Kernel_Name"]))
    rows.sort()
    marks = [s for s, _, n in rows if marker in n]
    if len(marks) < steps + 1:
        sys.exit(f"{len(marks)} launches of {marker!r}: need {steps + 1}")
    lo, hi = marks[-steps - 1], marks[-1]
    win = [(e - s, n) for s, e, n in rows if lo <= s < hi]
    per, fam = {}, dict.fromkeys(FAMILIES, 0.0)
    for d, n in win:
        k = short(n)
        if k is None:
            continue
        c = per.setdefault(k, [0, 0.0])
        c[0] += 1
        c[1] += d / 1e6
        if k == ADD:
            continue
        f = next(f for f in FAMILIES
                 if (f + "_kernel" if f.startswith("bn_") else f) in k)
        fam[f] += d / 1e6
    print(f"# {path}: {steps} steps, {(hi - lo) / 1e6 / steps:.2f} ms wall per "
          f"step, {len(win) / steps:.1f} kernels per step")
    print(f"{'calls/step':>10} {'ms/step':>9}  kernel")
    for k, (c, ms) in sorted(per.items(), key=lambda kv: -kv[1][1]):
        print(f"{c / steps:10.1f} {ms / steps:9.3f}  {k}")
    print(f"{'':>10} {'ms/step':>9}  family")
    for f in FAMILIES:
        print(f"{'':>10} {fam[f] / steps:9.3f}  {f}")
    print(f"{'':>10} {sum(fam.values()) / steps:9.3f}  BN and pool kernels")
    print(f"{'':>10} {sum(d for d, _ in win) / 1e6 / steps:9.3f}  all kernels")


if __name__ == "__main__":
    main()
