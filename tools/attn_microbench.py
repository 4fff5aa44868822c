"""Microbenchmark: fused MFMA attention vs torch SDPA at BERT shapes.

Measures forward-only and forward+backward time for the hand-written
gfx950 kernels (attention.hip / attention_bwd.hip) against torch SDPA
(AOTriton flash attention on ROCm). Run on a GPU box:

    python tools/attn_microbench.py [--iters N]

With --kv-splits the forward-only comparison of the split-KV path is run
instead (p = 0): attn_fwd, attn_fwd_split at each given count and torch
SDPA, alternated in one process, device-event times, median and min..max
per side, over the shapes of SPLIT_SHAPES:

    python tools/attn_microbench.py --kv-splits 2,4,8 [--rounds 7]
"""
import argparse
import math
import sys
import time

import torch

sys.path.insert(0, __file__.rsplit("/", 2)[0])

SHAPES = {
    # (B, H, S, D)
    "bert_base_s128": (32, 12, 128, 64),
    "bert_base_s512": (8, 12, 512, 64),
    "bert_large_s128": (16, 16, 128, 64),
    "gpt_s1024": (4, 16, 1024, 64),
}


# dropout-free forward shapes where the one-kernel grid may or may not fill
# the GPU; b32_h12_s128 is the control the dispatch rule never selects
SPLIT_SHAPES = {
    "b8_h12_s512": (8, 12, 512, 64),
    "b4_h16_s1024": (4, 16, 1024, 64),
    "b1_h12_s512": (1, 12, 512, 64),
    "b1_h12_s1024": (1, 12, 1024, 64),
    "b2_h16_s512": (2, 16, 512, 64),
    "b4_h12_s512": (4, 12, 512, 64),
    "b1_h16_s2048": (1, 16, 2048, 64),
    "b32_h12_s128": (32, 12, 128, 64),
    "b2_h16_s1024_d128": (2, 16, 1024, 128),
    "b1_h12_s1024_d128": (1, 12, 1024, 128),
}


def event_ms(fn, iters):
    """Device-event time of `iters` back-to-back calls, per call."""
    start = torch.cuda.Event(enable_timing=True)
    stop = torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / iters


def split_compare(counts, iters, rounds):
    import json
    import statistics
    from autodist_amd.ops import api
    from autodist_amd.ops.fused_attention import auto_kv_splits
    ext = api.ext()
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    results = []
    for name, (B, H, S, D) in SPLIT_SHAPES.items():
        scale = 1.0 / math.sqrt(D)
        q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
        k, v = torch.randn_like(q), torch.randn_like(q)
        sides = {"attn_fwd": lambda: ext.attn_fwd(q, k, v, scale),
                 "sdpa": lambda: torch.nn.functional
                 .scaled_dot_product_attention(q, k, v, scale=scale)}
        for n in counts:
            sides[f"split{n}"] = (
                lambda n=n: ext.attn_fwd_split(q, k, v, scale, None, n))
        times = {side: [] for side in sides}
        with torch.no_grad():
            for fn in sides.values():
                event_ms(fn, 10)                      # warm-up
            for _ in range(rounds):                   # sides alternated
                for side, fn in sides.items():
                    times[side].append(event_ms(fn, iters))
        row = {"shape": name, "B": B, "H": H, "S": S, "D": D,
               "grid": -(-S // (128 if S >= 256 else 64)) * B * H,
               "rule": auto_kv_splits(B, H, S, D, n_cu)}
        for side, ts in times.items():
            row[side] = {"med": round(statistics.median(ts), 4),
                         "min": round(min(ts), 4), "max": round(max(ts), 4)}
        results.append(row)
        print(row, flush=True)
    print("JSON:" + json.dumps(results))


def bench(fn, iters=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--kv-splits", default="",
                   help="comma-separated split counts: time the split-KV "
                        "forward against attn_fwd and SDPA instead")
    p.add_argument("--rounds", type=int, default=7,
                   help="alternated timing rounds per side (--kv-splits)")
    args = p.parse_args()
    if args.kv_splits:
        split_compare([int(n) for n in args.kv_splits.split(",")],
                      args.iters, args.rounds)
        return
    from autodist_amd.ops.fused_attention import FusedAttentionFn
    results = []
    for name, (B, H, S, D) in SHAPES.items():
        scale = 1.0 / math.sqrt(D)
        q = torch.randn(B, H, S, D, device="cuda", dtype=torch.bfloat16)
        k = torch.randn_like(q)
        v = torch.randn_like(q)
        dout = torch.randn_like(q)

        def sdpa_fwd():
            with torch.no_grad():
                torch.nn.functional.scaled_dot_product_attention(
                    q, k, v, scale=scale)

        def fused_fwd():
            with torch.no_grad():
                from autodist_amd.ops import api
                api.ext().attn_fwd(q, k, v, scale)

        qg = q.clone().requires_grad_(True)
        kg = k.clone().requires_grad_(True)
        vg = v.clone().requires_grad_(True)

        def sdpa_fb():
            o = torch.nn.functional.scaled_dot_product_attention(
                qg, kg, vg, scale=scale)
            torch.autograd.grad(o, (qg, kg, vg), dout)

        def fused_fb():
            o = FusedAttentionFn.apply(qg, kg, vg, scale, None, 0.0, 0)
            torch.autograd.grad(o, (qg, kg, vg), dout)

        def sdpa_fb_drop():
            o = torch.nn.functional.scaled_dot_product_attention(
                qg, kg, vg, scale=scale, dropout_p=0.1)
            torch.autograd.grad(o, (qg, kg, vg), dout)

        def fused_fb_drop():
            o = FusedAttentionFn.apply(qg, kg, vg, scale, None, 0.1, 777)
            torch.autograd.grad(o, (qg, kg, vg), dout)

        row = {
            "shape": name, "B": B, "H": H, "S": S, "D": D,
            "sdpa_fwd_ms": round(bench(sdpa_fwd, args.iters), 4),
            "fused_fwd_ms": round(bench(fused_fwd, args.iters), 4),
            "sdpa_fb_ms": round(bench(sdpa_fb, args.iters), 4),
            "fused_fb_ms": round(bench(fused_fb, args.iters), 4),
            "sdpa_fb_drop_ms": round(bench(sdpa_fb_drop, args.iters), 4),
            "fused_fb_drop_ms": round(bench(fused_fb_drop, args.iters), 4),
        }
        row["fwd_speedup"] = round(row["sdpa_fwd_ms"] / row["fused_fwd_ms"], 3)
        row["fb_speedup"] = round(row["sdpa_fb_ms"] / row["fused_fb_ms"], 3)
        row["fb_drop_speedup"] = round(
            row["sdpa_fb_drop_ms"] / row["fused_fb_drop_ms"], 3)
        results.append(row)
        print(row, flush=True)
    import json
    print("JSON:" + json.dumps(results))


if __name__ == "__main__":
    main()
