"""bench.py JSON contract (the driver's interface): one JSON line with the
BASELINE-named metric/config fields, whole-job aggregate value."""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.integration

REQUIRED = ["metric", "value", "unit", "n_gpus", "steps", "warmup",
            "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config"]


def _run_bench(args):
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "1", "--warmup", "0"] + args,
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    return json.loads(line)


def test_default_contract():
    out = _run_bench(["--batch-size", "2", "--image-size", "64"])
    for k in REQUIRED:
        assert k in out, f"missing field {k}"
    assert out["metric"].startswith("images/sec ResNet-50")
    assert out["n_gpus"] == 1 and out["steps"] == 1 and out["warmup"] == 0
    assert out["scaling"] == "weak" and out["higher_is_better"] is True
    assert out["data"] == "synthetic"
    assert out["config"]["model"] == "resnet50"
    assert out["config"]["parallelism"] == "dp1"
    assert out["value"] > 0 and out["ms_per_step"] > 0


def test_dump_outputs_repeatable(tmp_path):
    """--dump-outputs writes the last timed step's loss and parameter sample
    as float32 .npy, finite on the default timed path (hipGraph replay on a
    GPU); same arguments -> same inputs and same starting state of the
    dumped step, so two runs, or runs with another number of steps, dump
    identical arrays on CPU and the same loss on a GPU. --full is accepted
    and keeps the result line's contract."""
    import numpy as np
    dumps = []
    # "c" runs two more steps first: the dumped step must not depend on them
    for name, extra in (("a", []), ("b", ["--full"]), ("c", ["--steps", "3"])):
        d = tmp_path / name
        out = _run_bench(["--batch-size", "2", "--image-size", "64",
                          "--dump-outputs", str(d)] + extra)
        for k in REQUIRED:
            assert k in out, f"missing field {k}"
        files = sorted(p.name for p in d.iterdir())
        assert files == ["loss.npy", "params.npy"]
        arrs = {f: np.load(d / f) for f in files}
        for f, a in arrs.items():
            assert a.dtype == np.float32, (f, a.dtype)
            assert np.isfinite(a).all(), f
        assert arrs["loss.npy"].shape == (1,)
        assert sum(a.nbytes for a in arrs.values()) <= 64 * 1024 * 1024
        dumps.append(arrs)
    # The dumped step starts from the seeded state, so the CPU path is
    # bit-reproducible. On a GPU the loss, which the forward pass alone
    # computes, agrees to one bf16 rounding (bit-equal when measured). The
    # bf16 backward kernels sum with atomics, and this test's shape is too
    # ill-conditioned to bound their effect on the parameters: BatchNorm
    # over 8 samples has channels with next to no variance, rstd up to 316,
    # and updates of up to 14 in one step; two runs differed by 0.25 and by
    # 4.2 where the largest update was 8. At the benchmark's own shape
    # (batch 512, 224x224) two runs agreed to 4.4e-4, lr times one bf16
    # rounding of a gradient. So the parameters' difference is printed here.
    for other in dumps[1:]:
        for f in dumps[0]:
            a, b = dumps[0][f], other[f]
            print(f, "max |a-b|", float(np.abs(a - b).max()))
            if out["dtype"] == "fp32":
                assert np.array_equal(a, b), f
            elif f == "loss.npy":
                assert abs(float(a[0]) - float(b[0])) <= 2.0 ** -8 * a[0]


def test_bert_contract():
    out = _run_bench(["--model", "bert", "--batch-size", "2",
                      "--seq-len", "32"])
    assert out["metric"].startswith("sequences/sec BERT-base")
    assert out["config"]["seq_len"] == 32
    assert out["config"]["strategy"] == "Parallax"
