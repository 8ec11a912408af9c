"""bench.py's N > 1 path, run as the driver's scaling run would run it (two ranks, the same
rounds, transfers, run-time checks and C4 record), on CPU over gloo with an engine stand-in
(tests/bench_dist_driver.py). The GPU box has one GPU, so this is where the multi-rank loop is
exercised before the driver's N = 2..8 runs."""
import json
import os
import socket
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run(args, world=2):
    port = _free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=str(port), OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "bench_dist_driver.py")] + args,
                                      env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True))
    outs = [p.communicate(timeout=240) for p in procs]
    for p, (o, e) in zip(procs, outs):
        assert p.returncode == 0, e[-3000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1, outs[0][0][-2000:]
    assert not [l for l in outs[1][0].splitlines() if l.startswith("{")]  # rank 0 prints alone
    return json.loads(lines[0])


def test_c2_weak_line_with_c4_record():
    d = _run(["--gpus", "2", "--steps", "20", "--warmup", "5", "--frames", "512", "--c4-frames", "4096",
              "--cpu-seconds", "0", "--min-warm", "0", "--full"])
    assert d["n_gpus"] == 2 and d["steps"] == 20 and d["scaling"] == "weak"
    assert d["config"]["global_batch_frames"] == 1024 and "RCCL" in d["config"]["parallelism"]
    c4 = d["c4_strong"]
    assert c4["scaling"] == "strong" and c4["config"]["global_batch_frames"] == 4096
    assert c4["value"] > 0 and c4["ms_per_step"] > 0


def test_plain_line_and_dumped_outputs(tmp_path):
    """Without --full the line holds the headline alone (no C4 record, no kernel-only pass, no CPU
    baseline); --dump-outputs writes rank 0's last timed step, the same from run to run."""
    import numpy as np

    args = ["--gpus", "2", "--steps", "11", "--warmup", "5", "--frames", "512", "--min-warm", "0"]
    dumps = []
    for k in range(2):
        d = _run(args + ["--dump-outputs", str(tmp_path / f"run{k}")])
        assert d["steps"] == 11 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "GiB/s"
        assert d["higher_is_better"] is True and d["dtype"] == "u8" and "GiB/s" in d["metric"]
        assert "c4_strong" not in d and d["cpu_baseline"] is None and "kernel_avg_us" not in d["roofline"]
        dumps.append({f: np.load(tmp_path / f"run{k}" / f) for f in sorted(os.listdir(tmp_path / f"run{k}"))})
    assert sorted(dumps[0]) == ["digest_words.npy", "verdicts.npy"]
    for f, a in dumps[0].items():
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, dumps[1][f])
    # the stand-in engine's digest of rank 0: (frame length, rank + 1), verdict 0
    assert np.array_equal(dumps[0]["digest_words.npy"], np.tile([1500.0, 1.0], (512, 1)))
    assert dumps[0]["verdicts.npy"].shape == (512,) and not dumps[0]["verdicts.npy"].any()


def test_dump_outputs_samples_past_the_limit(tmp_path, monkeypatch):
    import numpy as np

    import bench

    monkeypatch.setattr(bench, "DUMP_LIMIT", 4000)
    big = np.arange(3000, dtype=np.int32).reshape(1500, 2)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / str(k)), {"big": big, "small": np.arange(7, dtype=np.uint8)})
    a, b = np.load(tmp_path / "0" / "big.npy"), np.load(tmp_path / "1" / "big.npy")
    assert a.dtype == np.float64 and a.shape == (250,) and np.array_equal(a, b) and (np.diff(a) > 0).all()
    s = np.load(tmp_path / "0" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, np.arange(7))
    assert sum(os.path.getsize(tmp_path / "0" / f) for f in os.listdir(tmp_path / "0")) <= 4000 + 2 * 128


def test_c4_config_line():
    d = _run(["--gpus", "2", "--config", "c4", "--steps", "7", "--warmup", "3", "--frames", "3001",
              "--cpu-seconds", "0"])
    assert d["scaling"] == "strong" and d["n_gpus"] == 2 and d["config"]["global_batch_frames"] == 3001


def test_long_region_rounds():
    # 64 steps: rounds 32, 16, 8, 8 over 5 streams; the run-time schedule assert covers them
    d = _run(["--gpus", "2", "--steps", "64", "--warmup", "7", "--frames", "256", "--no-c4", "--cpu-seconds", "0",
              "--min-warm", "0"])
    assert d["steps"] == 64 and "c4_strong" not in d


def test_gpu_seam_calls_torch_cuda():
    """The real seam (bench.GpuOps) calls torch.cuda / torch.distributed / seqs_amd directly,
    never back into bench.GPU (the CPU stand-ins above override every method, so the loop
    tests cannot see that)."""
    import ast
    import inspect

    import bench

    src = inspect.getsource(bench.GpuOps)
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, ast.Attribute) and isinstance(node.value, ast.Name):
            assert node.value.id != "GPU", f"GpuOps calls GPU.{node.attr}"
