"""Driver-contract tests for the benchmark scripts: they must run on
CPU with default-compatible flags and print ONE JSON line with the
agreed schema (the round driver invokes them verbatim)."""

import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

REPO = Path(__file__).parent.parent

REQUIRED_FIELDS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}

# The gloo/CPU rehearsals must stay on the CPU on machines that have GPUs
# too (a 1-GPU machine cannot give every rank of a world-2/4/8 launch its
# own device): hide the devices from the launched benchmark.
CPU_ONLY = {"HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""}


def _run(cmd, timeout=240, extra_env=None):
    env = dict(os.environ, PYTHONPATH=str(REPO) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    env.update(extra_env or {})
    proc = subprocess.run(
        cmd, cwd=REPO, capture_output=True, text=True, timeout=timeout, env=env
    )
    assert proc.returncode == 0, proc.stderr[-3000:]
    line = proc.stdout.strip().splitlines()[-1]
    return json.loads(line)


@pytest.mark.timeout(300)
def test_bench_default_contract_cpu():
    d = _run([sys.executable, "bench.py", "--steps", "6", "--warmup", "2",
              "--batch", "64", "--minibatches", "4"])
    assert REQUIRED_FIELDS <= set(d)
    assert d["metric"] == "train_samples_per_sec"
    assert d["n_gpus"] == 1 and d["steps"] == 6 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["config"]["model"] == "digits_mlp_64x32x10"
    assert d["config"]["global_batch"] == 64
    assert d["config"]["parallelism"] == "dp1"
    assert d["data"] == "synthetic"


@pytest.mark.timeout(300)
def test_bench_dump_outputs_and_full_cpu(tmp_path):
    """--dump-outputs writes the state left by the last timed step as
    float .npy files, reproducibly from the seeded inputs; --steps sets
    the number of timed optimizer steps; --full keeps the result line."""
    import numpy as np

    base = [sys.executable, "bench.py", "--gpus", "1", "--warmup", "2",
            "--batch", "64", "--minibatches", "4"]
    # CPU contract; test_bench_dump_outputs_gpu below runs the GPU engines
    cpu = CPU_ONLY
    a = _run(base + ["--steps", "6", "--dump-outputs", str(tmp_path / "a"), "--full"],
             extra_env=cpu)
    b = _run(base + ["--steps", "6", "--dump-outputs", str(tmp_path / "b")], extra_env=cpu)
    c = _run(base + ["--steps", "9", "--dump-outputs", str(tmp_path / "c")], extra_env=cpu)
    assert "stepwise+eager" == a["config"]["engine"]
    for d in (a, b, c):
        assert REQUIRED_FIELDS <= set(d)
        assert d["metric"] == "train_samples_per_sec" and d["ms_per_step"] > 0
    assert a["config"].get("full") is True and "full" not in b["config"]

    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["adam_m.npy", "adam_v.npy", "bfmirror.npy", "loss.npy",
                     "master.npy", "step_count.npy"]
    total = 0
    for name in names:
        xa, xb = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert xa.dtype in (np.float32, np.float64), (name, xa.dtype)
        assert np.isfinite(xa).all(), name
        # the CPU reference path is deterministic: same args, same outputs
        assert np.array_equal(xa, xb), name
        total += xa.nbytes
    assert total <= 64 * 2**20
    assert np.load(tmp_path / "a" / "master.npy").shape == (2608,)
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == a["config"]["final_loss"]
    # three more timed steps advance the device step counter by exactly three
    steps_a = float(np.load(tmp_path / "a" / "step_count.npy")[0])
    steps_c = float(np.load(tmp_path / "c" / "step_count.npy")[0])
    assert steps_c - steps_a == 3.0
    assert not np.array_equal(np.load(tmp_path / "c" / "master.npy"),
                              np.load(tmp_path / "a" / "master.npy"))


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("engine,label", [("auto", "fused+hipgraph4"),
                                          ("persistent", "persistent_steps_kernel")])
def test_bench_dump_outputs_gpu(tmp_path, engine, label):
    """--dump-outputs on the GPU engines: the fused step under hipGraph
    replay (graph chunks plus eager edges) and the persistent kernel's
    early return. Same arguments, same bits, from run to run."""
    import numpy as np
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs MI355X")
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "2",
           "--batch", "256", "--minibatches", "4", "--graph-steps", "4",
           "--engine", engine]
    a = _run(cmd + ["--dump-outputs", str(tmp_path / "a")])
    b = _run(cmd + ["--dump-outputs", str(tmp_path / "b")])
    assert a["config"]["engine"] == label and b["config"]["engine"] == label
    if engine == "auto":
        assert a["config"]["graph_replays_used"] == 2  # steps [4,8) and [8,12)
    names = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert names == ["adam_m.npy", "adam_v.npy", "bfmirror.npy", "loss.npy",
                     "master.npy", "step_count.npy"]
    for name in names:
        xa, xb = np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)
        assert xa.dtype in (np.float32, np.float64), (name, xa.dtype)
        assert np.isfinite(xa).all(), name
        assert np.array_equal(xa, xb), name
    assert float(np.load(tmp_path / "a" / "loss.npy")[0]) == a["config"]["final_loss"]
    assert np.abs(np.load(tmp_path / "a" / "adam_m.npy")).max() > 0


@pytest.mark.timeout(300)
def test_bench_serve_mode_rejects_dump_outputs(tmp_path):
    proc = subprocess.run(
        [sys.executable, "bench.py", "--mode", "serve", "--dump-outputs", str(tmp_path / "x")],
        cwd=REPO, capture_output=True, text=True, timeout=120)
    assert proc.returncode != 0 and "--dump-outputs" in proc.stderr
    assert not (tmp_path / "x").exists()


@pytest.mark.timeout(300)
def test_bench_world2_gloo_cpu():
    """The exact launch shape the driver uses for N>1, on gloo/CPU."""
    d = _run([
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
        "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
        "--master-port", "29590", "bench.py", "--gpus", "2", "--steps", "4",
        "--warmup", "1", "--batch", "32", "--minibatches", "4",
    ], extra_env=CPU_ONLY)
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 64


@pytest.mark.timeout(300)
def test_bench_resnet_contract_cpu():
    d = _run([sys.executable, "benchmarks/bench_resnet.py", "--steps", "2",
              "--warmup", "1", "--batch", "2", "--image-size", "32",
              "--classes", "4"], extra_env=CPU_ONLY)
    assert REQUIRED_FIELDS <= set(d)
    assert d["config"]["model"] == "resnet18"


@pytest.mark.timeout(420)
def test_bench_world4_gloo_cpu():
    """First-contact rehearsal for the driver's 4-GPU scaling point."""
    d = _run([
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
        "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
        "--master-port", "29591", "bench.py", "--gpus", "4", "--steps", "4",
        "--warmup", "1", "--batch", "16", "--minibatches", "4",
    ], timeout=400, extra_env=CPU_ONLY)
    assert d["n_gpus"] == 4
    assert d["config"]["parallelism"] == "dp4"
    assert d["config"]["global_batch"] == 64


@pytest.mark.timeout(600)
def test_bench_world8_gloo_cpu():
    """First-contact rehearsal for the driver's full-node scaling point."""
    d = _run([
        sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
        "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
        "--master-port", "29592", "bench.py", "--gpus", "8", "--steps", "2",
        "--warmup", "1", "--batch", "16", "--minibatches", "2",
    ], timeout=560, extra_env=CPU_ONLY)
    assert d["n_gpus"] == 8
    assert d["config"]["parallelism"] == "dp8"


@pytest.mark.timeout(300)
def test_bench_engine_label_truthful():
    """The engine label must say 'eager' when no graph replays happened
    in the timed region (a hipgraphG label on an eager
    timed region overstated what ran)."""
    d = _run([sys.executable, "bench.py", "--steps", "4", "--warmup", "1",
              "--batch", "32", "--minibatches", "4"])
    assert "eager" in d["config"]["engine"]  # CPU: graphs never capture
    assert d["config"].get("graph_replays_used", 0) == 0


@pytest.mark.timeout(420)
def test_bench_serve_mode_contract():
    """--mode serve reports the /predict p50 leg of the BASELINE metric
    through the real FastAPI app over HTTP."""
    d = _run([sys.executable, "bench.py", "--mode", "serve", "--steps", "40",
              "--warmup", "5"], timeout=400)
    assert d["metric"] == "predict_p50_ms"
    assert d["higher_is_better"] is False
    assert d["value"] > 0
    assert d["config"]["p99_ms"] >= d["value"]
    assert d["config"]["rps"] > 0


@pytest.mark.timeout(300)
def test_bench_persistent_engine_falls_back_cpu():
    """Unmet persistent-engine constraints must fall back per-engine,
    not kill the process."""
    d = _run([sys.executable, "bench.py", "--engine", "persistent", "--steps", "4",
              "--warmup", "1", "--batch", "48", "--minibatches", "4"])
    assert d["value"] > 0  # survived via fallback (48 % 128 != 0, CPU anyway)
