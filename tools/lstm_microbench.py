"""Microbenchmark: the LM1B recurrent stack through fused_lstmp (bf16 MFMA
cell kernels, ops/csrc/lstm_ops.hip) against the fp32 nn.LSTM call that
LM1BModel made before it, on one GPU.

Shape: B = 128, T = 20, E = 512, H = 2048, P = 512, 2 layers, fp32 input and
parameters. The fused side runs under bf16 autocast with backward() outside
the block, as bench.py does; the fp32 side runs outside autocast. Forward
alone and forward + backward are timed; the two sides alternate in one
process, `--rounds` times `--iters` calls between device events after
warm-up, and the median round and the min..max spread are reported. Needs a
GPU:
    python tools/lstm_microbench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, E, H, P, LAYERS = 128, 20, 512, 2048, 512, 2


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lstm_microbench needs a GPU")
    from autodist_amd.ops.fused_lstm import can_use_fused_lstmp, fused_lstmp
    torch.manual_seed(0)
    lstm = torch.nn.LSTM(E, H, num_layers=LAYERS, proj_size=P,
                         batch_first=True).cuda()
    x = torch.randn(B, T, E, device="cuda", requires_grad=True)
    w = torch.randn(B, T, P, device="cuda")
    assert can_use_fused_lstmp(x, lstm)

    def fused(backward):
        lstm.zero_grad(set_to_none=True)
        x.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out, _ = fused_lstmp(x, lstm)
            loss = (out.float() * w).sum()
        if backward:
            loss.backward()
        return loss

    def fp32(backward):
        lstm.zero_grad(set_to_none=True)
        x.grad = None
        out, _ = lstm(x)
        loss = (out * w).sum()
        if backward:
            loss.backward()
        return loss

    for _ in range(args.warmup):
        l_new, l_old = fused(True), fp32(True)
    torch.cuda.synchronize()
    rel = abs(l_new.item() - l_old.item()) / max(abs(l_old.item()), 1.0)
    print(f"loss fused {l_new.item():.4f} fp32 {l_old.item():.4f}")
    assert rel < 5e-2, (l_new.item(), l_old.item())
    rec = {"B": B, "T": T, "E": E, "H": H, "P": P, "layers": LAYERS}
    for name, bwd in (("fwd", False), ("fwd_bwd", True)):
        t_new, t_old = [], []
        for _ in range(args.rounds):
            t_new.append(_time(lambda: fused(bwd), args.iters))
            t_old.append(_time(lambda: fp32(bwd), args.iters))
        rec[name] = {"fused": _rounds(t_new), "fp32_nn_lstm": _rounds(t_old),
                     "speedup": round(statistics.median(t_old)
                                      / statistics.median(t_new), 3)}
    print(json.dumps(rec), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
