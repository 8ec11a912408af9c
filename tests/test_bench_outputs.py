"""bench.py's own command on the GPU, small: a plain run prints the headline line alone, and what
--dump-outputs writes is the last timed step's result, bit-exact against the CPU oracle."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path, oracle_lib):
    from oracle import coracle
    from seqs_amd import split_digests, synth

    steps, warmup, n = 7, 3, 1000
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", str(warmup), "--frames", str(n), "--min-warm", "0",
                        "--dump-outputs", str(tmp_path)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == steps and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "GiB/s"
    assert d["higher_is_better"] is True and d["dtype"] == "u8"
    # nothing that takes a run of its own
    assert d["cpu_baseline"] is None and "kernel_avg_us" not in d["roofline"]
    assert not {"c3", "c5_host", "small", "fill", "fcs", "small_host"} & set(d)

    words, st = np.load(tmp_path / "digest_words.npy"), np.load(tmp_path / "verdicts.npy")
    assert words.dtype == np.float64 and words.shape == (n, 2) and st.shape == (n,)
    # the last timed step digested batch (warmup + steps - 1) % 4, seeded 1 + that index
    buf, off, ln = synth.uniform_batch(n, 1500, seed=1 + (warmup + steps - 1) % 4)
    dig, est = coracle.digest_batch(buf, off, ln)
    crc, ipc, l4c = split_digests(words.astype(np.int64).astype(np.int32))
    assert np.array_equal(crc, dig["crc32"]) and np.array_equal(ipc, dig["ip_csum"])
    assert np.array_equal(l4c, dig["l4_csum"]) and np.array_equal(st.astype(np.uint8), est)
