"""Microbenchmark: the sharded vocab-parallel cross-entropy through the
ce_shard_* HIP kernels against the torch elementwise chain
(AUTODIST_VOCAB_CE=torch), on one GPU with a forced world-1 RCCL group.

Times VocabParallelProjection.loss forward + backward at one rank's share
of the LM1B benchmark at world 8: N = 2560 rows, D = 512, V_r = 99184 (a
multiple of 8) and 99183 (odd: padded row stride), fp32 hidden and
parameters under bf16 autocast. The two sides alternate in one process,
`--rounds` times `--iters` steps between device events after warm-up; the
median round and the min..max spread are reported. The new side calls
backward() outside the autocast block, as bench.py does. The OLD side
cannot: its backward fails there with a dtype error, so for the old side
only backward runs inside the block.

The kernels alone (stats + combine, bwd + partial sum) are also timed on a
logits buffer of the layout the function builds, and reported with the
bytes they need, counted from the shapes, over their time. Needs a GPU:
    python tools/ce_shard_microbench.py [--json out.json]
"""
import argparse
import json
import os
import socket
import statistics
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N, D = 2560, 512
SHARDS = [99184, 99183]


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
        raise SystemExit("ce_shard_microbench needs a GPU")
    os.environ["AUTODIST_FORCE_COLLECTIVES"] = "1"
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}",
                            rank=0, world_size=1)
    from autodist_amd.ops import api as ops_api
    from autodist_amd.parallel.vocab_parallel import VocabParallelProjection
    ext = ops_api.ext()
    print("old side: backward() inside the autocast block (it fails outside); "
          "new side: backward() outside, as in bench.py")
    results = []
    for v in SHARDS:
        torch.manual_seed(v)
        proj = VocabParallelProjection(v, D, rank=0, world_size=1).cuda()
        hidden = torch.randn(N, D, device="cuda", requires_grad=True)
        targets = torch.randint(0, v, (N,), device="cuda")

        def step(side):
            os.environ["AUTODIST_VOCAB_CE"] = side
            proj.zero_grad(set_to_none=True)
            hidden.grad = None
            with torch.autocast("cuda", dtype=torch.bfloat16):
                loss = proj.loss(hidden, targets)
                if side == "torch":
                    loss.backward()
            if side == "hip":
                loss.backward()
            return loss

        for _ in range(args.warmup):
            l_new, l_old = step("hip"), step("torch")
        torch.cuda.synchronize()
        assert abs(l_new.item() - l_old.item()) < 1e-2, (l_new, l_old)
        t_new, t_old = [], []
        for _ in range(args.rounds):
            t_new.append(_time(lambda: step("hip"), args.iters))
            t_old.append(_time(lambda: step("torch"), args.iters))
        os.environ.pop("AUTODIST_VOCAB_CE")

        # the kernels alone, on the function's own layout
        ld = (v + 7) // 8 * 8
        logits = torch.empty(N, ld, dtype=torch.bfloat16,
                             device="cuda")[:, :v]
        logits.copy_(torch.randn(N, v, device="cuda") * 3)
        dloss = torch.full((N,), 1.0 / N, device="cuda")
        lse2 = ext.ce_shard_combine(
            ext.ce_shard_stats(logits, targets, 0)[None])[1]

        def fwd_k():
            ext.ce_shard_combine(ext.ce_shard_stats(logits, targets, 0)[None])

        def bwd_k():
            ext.ce_shard_bwd(logits, targets, 0, lse2, dloss)

        for _ in range(args.warmup):
            fwd_k()
            bwd_k()
        t_f = [_time(fwd_k, args.iters) for _ in range(args.rounds)]
        t_b = [_time(bwd_k, args.iters) for _ in range(args.rounds)]
        # needed bytes: forward reads the shard once; backward reads it and
        # writes dlogits, and writes + re-reads the fp32 partial rows
        shard = N * v * 2
        chunks = -(-N // ext.CE_BWD_ROWS)
        strips = -(-v // ext.CE_STRIP_COLS)
        part = chunks * strips * ext.CE_STRIP_COLS * 4
        fwd_bytes, bwd_bytes = shard, 2 * shard + 2 * part
        f_ms, b_ms = statistics.median(t_f), statistics.median(t_b)
        rec = {"N": N, "D": D, "V_r": v, "ld": ld,
               "new_step": _rounds(t_new), "old_step": _rounds(t_old),
               "speedup": round(statistics.median(t_old)
                                / statistics.median(t_new), 3),
               "fwd_kernels": _rounds(t_f), "bwd_kernels": _rounds(t_b),
               "fwd_bytes": fwd_bytes, "bwd_bytes": bwd_bytes,
               "fwd_gbps": round(fwd_bytes / f_ms / 1e6, 1),
               "bwd_gbps": round(bwd_bytes / b_ms / 1e6, 1)}
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del proj, hidden, logits
        torch.cuda.empty_cache()
    dist.destroy_process_group()
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
