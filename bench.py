"""Driver benchmark for the BASELINE configs.

Default (no flags): ResNet-50 data-parallel training, images/sec — the
headline metric in BASELINE.json ("images/sec ResNet-50 AllReduce at
1/2/4/8 MI355X; scaling efficiency"). bf16 autocast compute, fp32 params,
synthetic data, random-init weights, AllReduce strategy over RCCL/xGMI.

--model selects the other BASELINE configs (each emits the same JSON
contract, driver-verifiable):
  bert   — BERT-base Parallax (config #3), sequences/sec
  ncf    — NCF PartitionedPS, sparse embedding push/pull (config #4),
           samples/sec
  lm1b   — LM1B LSTM, simulator-selected strategy (config #5), words/sec

Usage:  python bench.py [--model M] --gpus N --steps K --warmup W
                        [--dump-outputs DIR] [--full]
A plain run sets up, warms up, times the K steps and prints the result
line. --dump-outputs DIR also writes the last timed step's loss and a
seeded sample of the updated parameters as DIR/*.npy. The inputs are
seeded, and with --dump-outputs the last timed step starts again from the
seeded initial training state (see make_state_restorer), so two runs or two
builds can be compared output for output. --full is the
place for secondary measurements and checks; none exist yet.
The driver launches N>1 via torch.distributed.run (one rank per GPU); run
standalone and it re-execs itself under the launcher.
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=20)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--model", default="resnet50",
                   choices=["resnet50", "resnet101", "bert", "ncf", "lm1b"])
    p.add_argument("--batch-size", type=int, default=None,
                   help="per-GPU batch (weak scaling; default per model)")
    p.add_argument("--strategy", default=None,
                   help="strategy builder name (default per model)")
    p.add_argument("--bucket-mb", type=int, default=25)
    p.add_argument("--seq-len", type=int, default=None)
    p.add_argument("--image-size", type=int, default=224)
    p.add_argument("--no-channels-last", action="store_true")
    p.add_argument("--no-fused-bn", action="store_true",
                   help="disable the hand-written gfx950 fused BN kernels")
    p.add_argument("--hipgraph", choices=["auto", "on", "off"], default="auto",
                   help="capture the train step in a hipGraph (auto: on for "
                        "graph-safe models)")
    p.add_argument("--force-collectives", action="store_true",
                   help="execute real RCCL collectives even at world 1 "
                        "(1-GPU hardware validation of the comm path)")
    p.add_argument("--no-tunableop", action="store_true",
                   help="disable PYTORCH_TUNABLEOP GEMM algo tuning")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps write what the last timed "
                        "step computed (its loss, and a fixed seeded sample "
                        "of the parameters it updated) as DIR/<name>.npy; "
                        "that step starts from the seeded initial state")
    p.add_argument("--full", action="store_true",
                   help="also run the benchmark's secondary measurements and "
                        "checks; a plain run does only what the headline "
                        "figure needs")
    return p.parse_args()


DUMP_PARAM_ELEMS = 1 << 22  # fp32 sample of the parameters: 16 MiB


def dump_outputs(out_dir, loss, model):
    """Write the last timed step's results as float32 .npy files: the loss
    it returned and the parameters it updated in place. Parameters are
    sampled at fixed seeded positions (each tensor gets a share of
    DUMP_PARAM_ELEMS proportional to its size, in named_parameters order),
    so two builds run with the same arguments dump the same elements."""
    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"),
            loss.detach().float().cpu().numpy().reshape(-1))
    params = [p for _, p in model.named_parameters()]
    total = sum(p.numel() for p in params)
    rng = np.random.default_rng(20260914)
    chunks = []
    for p in params:
        flat = p.detach().reshape(-1)
        n = flat.numel()
        if total > DUMP_PARAM_ELEMS:
            k = min(n, max(1, DUMP_PARAM_ELEMS * n // total))
            idx = np.sort(rng.integers(0, n, size=k))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        chunks.append(flat.float().cpu().numpy())
    np.save(os.path.join(out_dir, "params.npy"), np.concatenate(chunks))


def make_state_restorer(engine, model):
    """Snapshot the seeded training state (parameters, module buffers,
    optimizer state) right after the workload is built and return a function
    that puts it back in place, or None where the engine keeps state this
    cannot reach (PS master copies, sparse and partitioned shards).

    --dump-outputs restores it before the last timed step, so that step's
    outputs depend on the seeded inputs alone. Without that they also carry
    the summation-order noise of every earlier step (the bf16 conv and
    pooling backward kernels accumulate with atomics), which ResNet-50 at
    lr 0.1 grows by about 1.5x per step: after 28 steps two runs of one
    build differed by 1.5 in the loss. Optimizer state is created lazily in
    the first step; state that does not exist yet is restored as zeros,
    which for the momentum, moment and step-count buffers used here is the
    state before the first step."""
    if not engine.buckets or not all(p.bucketed for p in engine.var_plans):
        return None
    saved = [(b.flat_param, b.flat_param.clone()) for b in engine.buckets]
    saved += [(t, t.clone()) for t in model.buffers()]
    known = {id(t) for t, _ in saved}
    for b in engine.buckets:
        for t in b.state.values():
            if torch.is_tensor(t) and id(t) not in known:
                saved.append((t, t.clone()))
                known.add(id(t))

    def restore():
        with torch.no_grad():
            for t, s in saved:
                t.copy_(s)
            for b in engine.buckets:
                for t in b.state.values():
                    if torch.is_tensor(t) and id(t) not in known:
                        t.zero_()
    return restore


def _miopen_user_db():
    return os.environ.get("MIOPEN_USER_DB_PATH") or os.path.join(
        os.path.expanduser("~"), ".config", "miopen")


def _find_marker(args):
    """File that records a completed exhaustive MIOpen find for this conv
    configuration. It lives inside MIOpen's user db directory, so it goes
    away together with the find results it stands for."""
    key = "_".join(str(v) for v in (
        args.model, args.batch_size or "default", args.image_size,
        int(not args.no_channels_last), int(not args.no_fused_bn),
        torch.__version__))
    return os.path.join(_miopen_user_db(), f"autodist_amd_find_{key}.done")


def relaunch_under_torchrun(args):
    """Self-relaunch with one rank per GPU when run standalone."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run",
           "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.abspath(__file__)] + sys.argv[1:]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    os.execvpe(sys.executable, cmd, os.environ)


def _make_engine(model, opt, strategy_name, rank, world, device, bucket_mb):
    from autodist_amd import strategy as strat
    from autodist_amd.graph_item import GraphItem
    from autodist_amd.parallel.engine import DistributedEngine
    from autodist_amd.resource_spec import ResourceSpec

    g = GraphItem()
    g.extend_model(model)
    g.extend_optimizer_info(opt)
    builder = getattr(strat, strategy_name)()
    strategy = builder.build(g, ResourceSpec())
    if len(strategy.graph_config.replicas) != world:
        strategy.graph_config.replicas = [
            f"127.0.0.1:GPU:{r}" for r in range(world)]
    engine = DistributedEngine(g, strategy, rank=rank, world_size=world,
                               device=device,
                               bucket_bytes=bucket_mb * 1024 * 1024)
    engine.setup()
    return engine


def build_resnet(args, device, rank, world, use_cuda):
    from autodist_amd.models import resnet
    strategy_name = args.strategy or "AllReduce"
    B = args.batch_size or 512
    fused = use_cuda and not args.no_fused_bn
    model = getattr(resnet, args.model)(num_classes=1000, fused=fused)
    model = model.to(device)
    channels_last = use_cuda and not args.no_channels_last
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    opt = torch.optim.SGD(model.parameters(), lr=0.1, momentum=0.9,
                          weight_decay=1e-4)
    engine = _make_engine(model, opt, strategy_name, rank, world, device,
                          args.bucket_mb)
    x = torch.randn(B, 3, args.image_size, args.image_size, device=device)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    y = torch.randint(0, 1000, (B,), device=device)
    loss_fn = torch.nn.CrossEntropyLoss()

    def step():
        opt.zero_grad()
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16,
                            enabled=use_cuda):
            loss = loss_fn(model(x), y)
        loss.backward()
        opt.step()
        return loss

    pretty = "ResNet-50" if args.model == "resnet50" else args.model
    return dict(step=step, engine=engine, model=model, items_per_step=B,
                metric=f"images/sec {pretty} {strategy_name}",
                unit="images/sec", graph_safe=True,
                config={"model": args.model, "global_batch": world * B,
                        "seq_len": None, "parallelism": f"dp{world}",
                        "strategy": strategy_name,
                        "image_size": args.image_size})


def build_bert(args, device, rank, world, use_cuda):
    """BASELINE config #3: BERT-base Parallax (hybrid PS + AllReduce).
    Reference workload: examples/benchmark/bert.py (TF-model-garden)."""
    from autodist_amd.models import bert
    strategy_name = args.strategy or "Parallax"
    B = args.batch_size or 32
    S = args.seq_len or 128
    model = bert.bert_base().to(device)
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=0.01)
    engine = _make_engine(model, opt, strategy_name, rank, world, device,
                          args.bucket_mb)
    vocab = model.bert.cfg.vocab_size
    ids = torch.randint(0, vocab, (B, S), device=device)
    labels = ids.clone()
    labels[:, ::2] = -100  # predict every other position (synthetic MLM)
    nsp = torch.randint(0, 2, (B,), device=device)

    def step():
        opt.zero_grad()
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16,
                            enabled=use_cuda):
            loss = model.loss(ids, labels, nsp)
        loss.backward()
        opt.step()
        return loss

    return dict(step=step, engine=engine, model=model, items_per_step=B,
                metric=f"sequences/sec BERT-base {strategy_name}",
                unit="sequences/sec", graph_safe=True,
                config={"model": "bert_base", "global_batch": world * B,
                        "seq_len": S, "parallelism": f"dp{world}",
                        "strategy": strategy_name})


def build_ncf(args, device, rank, world, use_cuda):
    """BASELINE config #4: NCF PartitionedPS with sparse-embedding
    push/pull. Reference workload: examples/benchmark/ncf.py."""
    from autodist_amd.models.ncf import ncf_movielens
    strategy_name = args.strategy or "PartitionedPS"
    B = args.batch_size or 4096
    model = ncf_movielens(sparse=True).to(device)
    opt = torch.optim.SGD(model.parameters(), lr=0.05)
    engine = _make_engine(model, opt, strategy_name, rank, world, device,
                          args.bucket_mb)
    users = torch.randint(0, 138493, (B,), device=device)
    items = torch.randint(0, 26744, (B,), device=device)
    labels = torch.randint(0, 2, (B,), device=device)

    def step():
        opt.zero_grad()
        loss = model.loss(users, items, labels)
        loss.backward()
        opt.step()
        return loss

    return dict(step=step, engine=engine, model=model, items_per_step=B,
                metric=f"samples/sec NCF {strategy_name}",
                unit="samples/sec", graph_safe=False,  # sparse/PS host logic
                config={"model": "ncf_movielens", "global_batch": world * B,
                        "seq_len": None, "parallelism": f"dp{world}",
                        "strategy": strategy_name})


def build_lm1b(args, device, rank, world, use_cuda):
    """BASELINE config #5: LM1B LSTM LM with the simulator-selected
    strategy. Reference workload: examples/lm1b/lm1b_train.py."""
    from autodist_amd.models.lm1b import lm1b_full
    strategy_name = args.strategy or "AutoStrategy"
    B = args.batch_size or 128
    S = args.seq_len or 20
    # vocab-parallel tied softmax (parallel/vocab_parallel.py): the 793k x
    # 512 projection+CE shards across ranks (3 tiny collectives instead of
    # full-vocab logits); exact-match vs dense CE is test-covered
    model = lm1b_full(sharded_softmax=True).to(device)
    opt = torch.optim.Adagrad(model.parameters(), lr=0.2)
    engine = _make_engine(model, opt, strategy_name, rank, world, device,
                          args.bucket_mb)
    vocab = model.emb.num_embeddings
    tokens = torch.randint(0, vocab, (B, S), device=device)
    targets = torch.randint(0, vocab, (B, S), device=device)

    def step():
        opt.zero_grad()
        with torch.autocast(device_type="cuda", dtype=torch.bfloat16,
                            enabled=use_cuda):
            loss = model.loss(tokens, targets)
        loss.backward()
        opt.step()
        return loss

    return dict(step=step, engine=engine, model=model, items_per_step=B * S,
                metric=f"words/sec LM1B {strategy_name}",
                unit="words/sec", graph_safe=False,  # cuDNN-style LSTM
                config={"model": "lm1b_lstm", "global_batch": world * B,
                        "seq_len": S, "parallelism": f"dp{world}",
                        "strategy": strategy_name, "vocab": vocab,
                        "softmax": "vocab_parallel"})


BUILDERS = {"resnet50": build_resnet, "resnet101": build_resnet,
            "bert": build_bert, "ncf": build_ncf, "lm1b": build_lm1b}


def main():
    args = parse_args()
    if args.force_collectives:
        os.environ["AUTODIST_FORCE_COLLECTIVES"] = "1"
    if not args.no_tunableop:
        # hipBLASLt/rocBLAS GEMM algo tuning (per-shape, runs during the
        # untimed warmup; +1.8% measured on BERT-base). Results go to /tmp
        # so repo snapshots stay clean.
        os.environ.setdefault("PYTORCH_TUNABLEOP_ENABLED", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_TUNING", "1")
        os.environ.setdefault("PYTORCH_TUNABLEOP_FILENAME",
                              "/tmp/tunableop.csv")
    if args.gpus > 1 and "RANK" not in os.environ:
        relaunch_under_torchrun(args)

    rank = int(os.environ.get("RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    use_cuda = torch.cuda.is_available()
    # modulo device count: lets an N-rank job run on fewer GPUs (e.g. the
    # RCCL-validation mode: 2 ranks sharing the single leased MI355X)
    device = torch.device(
        "cuda",
        int(os.environ.get("LOCAL_RANK", 0)) % torch.cuda.device_count()) \
        if use_cuda else torch.device("cpu")
    if use_cuda:
        torch.cuda.set_device(device)
        # Exhaustive MIOpen find (~6 min for the ResNet-50 conv configs in
        # the first warmup step). Without it MIOpen's immediate mode picks
        # naive wrw kernels: 214 img/s vs 8458 measured. The find leaves its
        # picks in MIOpen's user find-db under $HOME, where immediate mode
        # finds them, but a find request re-benchmarks every solver in each
        # new process (~2 min measured with all kernels cached). So the
        # find runs once per configuration (build() does it on a GPU
        # machine) and later runs read its results in immediate mode.
        find_marker = _find_marker(args)
        torch.backends.cudnn.benchmark = not os.path.exists(find_marker)
        torch.backends.cuda.matmul.allow_tf32 = False
        if args.hipgraph != "off":
            # The engine's post-accumulate-grad hooks keep each parameter's
            # AccumulateGrad node alive, and such a node runs for good on the
            # stream that was current when it was made. Made on the default
            # stream, it put every gradient accumulation of the captured
            # step on a branch beside the capture stream, which went on to
            # reuse the gradient buffers that branch still read: the replayed
            # steps diverged to NaN. So the workload is set up, warmed up and
            # captured on one side stream.
            run_stream = torch.cuda.Stream(device)
            torch.cuda.set_stream(run_stream)

    torch.manual_seed(1234)
    wl = BUILDERS[args.model](args, device, rank, world, use_cuda)
    step, engine = wl["step"], wl["engine"]
    # PS rounds and sparse sync involve host-side queue state that a graph
    # replay would freeze — never capture those
    has_host_sync = any(sh.kind == "ps" for p in engine.var_plans
                        for sh in p.shards) \
        or any(p.sparse for p in engine.var_plans)
    wl["graph_safe"] = wl["graph_safe"] and not has_host_sync
    restore_state = make_state_restorer(engine, wl["model"]) \
        if args.dump_outputs else None

    import torch.distributed as dist

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if use_cuda:
            torch.cuda.synchronize(device)

    # hipGraph capture: the per-step kernel chain is launch-bound in eager
    # mode; replaying a captured graph removes host launch + python overhead
    # entirely. Capturing RCCL collectives SEGFAULTS in this ROCm 7.2 stack
    # (hipGraph capture_end crash, measured 2026-09-14), so auto-capture is
    # gated to runs with no active collectives; --hipgraph on forces a try.
    use_graph = use_cuda and (args.hipgraph == "on" or
                              (args.hipgraph == "auto" and wl["graph_safe"]
                               and not engine.collectives_active))
    run_step = step
    for _ in range(args.warmup):
        step()
    if use_graph:
        try:
            for _ in range(2):
                step()
            if world > 1:
                barrier_sync()  # all ranks enter capture together
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=run_stream):
                static_loss = step()
            graph.replay()
            torch.cuda.synchronize(device)
            assert bool(torch.isfinite(static_loss).item()), "graph NaN"
            run_step = graph.replay
            if rank == 0:
                print(f"# hipGraph capture OK (loss {static_loss.item():.3f})",
                      file=sys.stderr)
        except Exception as exc:  # noqa: BLE001 - fall back to eager
            print(f"# hipGraph capture failed, eager fallback: {exc}",
                  file=sys.stderr)
            run_step = step
    barrier_sync()
    t0 = time.perf_counter()
    last_loss = None
    for i in range(args.steps):
        if restore_state is not None and i == args.steps - 1:
            restore_state()  # a few device copies, ordered on the stream
        last_loss = run_step()
    barrier_sync()
    dt = time.perf_counter() - t0
    if run_step is not step:
        last_loss = static_loss  # a graph replay rewrites the captured loss
    # MAX elapsed over ranks
    if world > 1:
        t = torch.tensor([dt], dtype=torch.float64,
                         device=device if use_cuda else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    engine.drain()
    if args.dump_outputs and rank == 0 and last_loss is not None:
        dump_outputs(args.dump_outputs, last_loss, wl["model"])

    if rank == 0:
        value = world * wl["items_per_step"] * args.steps / dt
        # MIOpen find-cache sanity: with a cold find
        # cache and too little warmup, immediate-mode picks naive wrw conv
        # kernels and the metric silently collapses ~40x (measured 214 vs
        # 8458 img/s). Flag the anomaly instead of reporting it silently.
        if use_cuda and args.model.startswith("resnet"):
            per_img_ms = dt / args.steps * 1e3 / wl["items_per_step"]
            if per_img_ms > 0.6:  # healthy: ~0.12 ms/img (b512, MI355X)
                print(f"# WARNING: {per_img_ms:.2f} ms/image is ~5x+ off the "
                      f"expected MI355X rate — MIOpen likely missed its "
                      f"exhaustive find (cold cache / too few warmup steps);"
                      f" rerun with --warmup >= 5", file=sys.stderr)
                if os.path.exists(find_marker):
                    os.remove(find_marker)  # next run repeats the find
            elif torch.backends.cudnn.benchmark:
                os.makedirs(os.path.dirname(find_marker), exist_ok=True)
                with open(find_marker, "w") as f:
                    f.write("exhaustive find done\n")
        result = {
            "metric": wl["metric"],
            "value": round(value, 2),
            "unit": wl["unit"],
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16" if use_cuda else "fp32",
            "data": "synthetic",
            "config": wl["config"],
        }
        print(json.dumps(result))


if __name__ == "__main__":
    main()
