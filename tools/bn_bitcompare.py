"""Bit comparison of the fused BN entry points between two builds.

    python tools/bn_bitcompare.py --root TREE_A --dump a.npz
    python tools/bn_bitcompare.py --root TREE_B --dump b.npz
    python tools/bn_bitcompare.py --compare a.npz b.npz

--dump runs, on a GPU, every BN entry point that both builds have on seeded
inputs at the shapes below (bf16 and fp32, with and without residual, with the
packed mask and without; one shape past the apply grid cap) with the extension
found under --root, and stores every output as raw bits. --compare needs no
GPU: np.array_equal on every array, and exit status 1 if any differs or the
two files do not hold the same names.
"""
import argparse
import os
import sys

import numpy as np

# (C, M, dtype): tx_count 1 with a ragged block; tx_count 3 (not a divisor of
# 256); a reduce grid-stride loop with a tail; grid_c = 2; an apply grid past
# its cap with main trips and single rows; the same at rows_per_blk = 1
SHAPES = [(8, 257, "bf16"), (24, 1000, "fp32"), (64, 6149, "bf16"),
          (48, 1000, "fp32"), (2056, 70, "bf16"), (256, 140011, "bf16"),
          (2048, 16500, "bf16")]
EPS = 1e-5


def _bits(t):
    import torch
    t = t.detach().contiguous()
    if t.dtype == torch.bfloat16:
        t = t.view(torch.int16)
    return t.cpu().numpy()


def dump(root, path):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from autodist_amd.ops import api
    e = api.ext()
    out = {}

    def nhwc(t2d):
        M, C = t2d.shape
        return t2d.view(1, M, 1, C).permute(0, 3, 1, 2)

    for C, M, dt in SHAPES:
        dtype = torch.bfloat16 if dt == "bf16" else torch.float32
        g = torch.Generator(device="cuda").manual_seed(1000 * C + M)
        rnd = lambda *s: torch.randn(*s, generator=g, device="cuda")  # noqa
        x, res, zd = (nhwc(rnd(M, C).to(dtype)) for _ in range(3))
        dy, dy_b = (nhwc(rnd(M, C).to(dtype)) for _ in range(2))
        w, wd = (torch.rand(C, generator=g, device="cuda") + 0.5
                 for _ in range(2))
        b, bd, rm0 = rnd(C), rnd(C), rnd(C)
        rv0 = torch.rand(C, generator=g, device="cuda") + 0.5
        key = f"C{C}_M{M}_{dt}"

        def put(name, tensors):
            for i, t in enumerate(tensors):
                out[f"{key}/{name}/{i}"] = _bits(t)

        for relu in (False, True):
            for r in (None, res):
                tag = f"relu{int(relu)}_res{int(r is not None)}"
                rm, rv = rm0.clone(), rv0.clone()
                f = e.bn_fwd_train(x, w, b, rm, rv, r, EPS, 0.1, relu, None)
                put(f"bn_fwd_train_{tag}", list(f) + [rm, rv])
                bw = e.bn_bwd(x, dy, f[0], f[1], f[2], w, relu, r is not None,
                              None)
                put(f"bn_bwd_{tag}", bw)
        for r in (None, res):
            tag = f"res{int(r is not None)}"
            rm, rv = rm0.clone(), rv0.clone()
            y, sm, sr, mask = e.bn_fwd_train_mask(x, w, b, rm, rv, r, EPS, 0.1,
                                                  True, None)
            put(f"bn_fwd_train_mask_{tag}", [y, sm, sr, mask, rm, rv])
            put(f"bn_bwd_mask_{tag}", e.bn_bwd_mask(
                x, dy, mask, sm, sr, w, True, r is not None, None))
            put(f"bn_bwd_mask_join_{tag}", e.bn_bwd_mask_join(
                x, dy, dy_b, mask, sm, sr, w, None))
        rms = [rm0.clone() for _ in range(2)]
        rvs = [rv0.clone() for _ in range(2)]
        f = e.bn_fwd_train_add_bn(x, zd, w, b, rms[0], rvs[0], EPS, 0.1, None,
                                  wd, bd, rms[1], rvs[1], EPS, 0.2, None)
        put("bn_fwd_train_add_bn", list(f) + rms + rvs)
        # the backward of that tail as the older build spells it
        j = e.bn_bwd_mask_join(x, dy, dy_b, f[1], f[2], f[3], w, None)
        put("add_bn_bwd_z", j)
        put("add_bn_bwd_zd", e.bn_bwd(zd, j[3], j[3], f[4], f[5], wd, False,
                                      False, None))
        if hasattr(e, "BN_JOIN2_U"):
            # and in one call; compared under the older spelling's names
            j2 = e.bn_bwd_mask_join(x, dy, dy_b, f[1], f[2], f[3], w, None,
                                    zd, f[4], f[5], wd, None)
            put("add_bn_bwd_joint_z", j2[:4])
            put("add_bn_bwd_joint_zd", j2[4:])
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"{len(out)} arrays from {len(SHAPES)} shapes -> {path}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    # a joint-backward output is compared with the two-call output it must
    # equal when only one of the builds has the joint entry point
    alias = lambda k: k.replace("add_bn_bwd_joint_", "add_bn_bwd_")  # noqa
    names_a = {k for k in a.files if "joint" not in k}
    names_b = {k for k in b.files if "joint" not in k}
    bad = sorted(names_a ^ names_b)
    if bad:
        print("names that only one file has:", bad)
    n = 0
    for k in sorted(set(a.files) | set(b.files)):
        ka = k if k in a.files else alias(k)
        kb = k if k in b.files else alias(k)
        if ka not in a.files or kb not in b.files:
            continue
        n += 1
        if not np.array_equal(a[ka], b[kb]):
            bad.append(k)
            print(f"DIFFERS {k}: {int((a[ka] != b[kb]).sum())} of "
                  f"{a[ka].size} elements")
    print(f"{n} arrays compared, {len(bad)} mismatches")
    return 1 if bad else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(
        os.path.abspath(__file__))), help="tree whose extension is loaded")
    ap.add_argument("--dump", metavar="FILE.npz")
    ap.add_argument("--compare", nargs=2, metavar=("A.npz", "B.npz"))
    args = ap.parse_args()
    if args.dump:
        dump(args.root, args.dump)
    if args.compare:
        sys.exit(compare(*args.compare))


if __name__ == "__main__":
    main()
