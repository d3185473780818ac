"""bench.py --dump-outputs: what the timed path computed in its last step, written as .npy so that two builds of the
project can be compared output for output.  CPU tier: the writer (row cap, seeded row choice, dtype) and the argument
checks; GPU tier: two runs with different --steps / --warmup write the same file, and it holds exactly the samples
a caller of the timed path receives for the bench's seeded model and base samples."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import bench

ROOT = Path(__file__).resolve().parents[1]


def test_dump_keeps_a_small_batch_whole(tmp_path):
    x = torch.randn(1000, 16)
    bench.dump_outputs(tmp_path, x)
    got = np.load(tmp_path / "samples.npy")
    assert got.dtype == np.float32 and np.array_equal(got, x.numpy())


def test_dump_of_a_large_batch_is_a_fixed_sample_under_the_cap(tmp_path):
    n = bench.DUMP_MAX_ROWS + 12345
    x = torch.arange(n, dtype=torch.float32).view(n, 1).repeat(1, 16)        # row i holds i: the rows kept are readable
    bench.dump_outputs(tmp_path / "a", x)
    bench.dump_outputs(tmp_path / "b", x.clone())
    a, b = np.load(tmp_path / "a" / "samples.npy"), np.load(tmp_path / "b" / "samples.npy")
    assert a.shape == (bench.DUMP_MAX_ROWS, 16) and np.array_equal(a, b)
    rows = a[:, 0].astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < n     # distinct rows, in row order
    assert (tmp_path / "a" / "samples.npy").stat().st_size < 64 * 10 ** 6


@pytest.mark.parametrize("args", [["--steps", "0"], ["--warmup", "-1"]])
def test_bench_refuses_a_step_count_it_cannot_time(args):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=300,
                       cwd=str(ROOT))
    assert r.returncode == 2 and "--steps must be >= 1" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_dumped_samples_are_the_timed_paths_result_whatever_the_step_count(tmp_path, built_library):
    assert torch.cuda.is_available(), "the gpu tier needs a GPU"
    B = 4096
    recs = []
    for name, steps, warmup in (("a", "1", "0"), ("b", "3", "2")):
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", steps, "--warmup", warmup, "--batch", str(B),
               "--cpu-batch", "0", "--no-extras", "--dump-outputs", str(tmp_path / name)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(ROOT))
        assert r.returncode == 0, r.stderr[-3000:]
        recs.append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1]))
    assert [rec["steps"] for rec in recs] == [1, 3]
    a, b = np.load(tmp_path / "a" / "samples.npy"), np.load(tmp_path / "b" / "samples.npy")
    assert a.dtype == np.float32 and a.shape == (B, bench.DIM) and np.isfinite(a).all()
    assert np.array_equal(a, b)
    # the same solve in this process: the bench's seeded model and base samples, the timed call
    from flowfusion_amd import _native
    dev = torch.device("cuda", 0)
    sm = bench.build_model(dev)
    z = _native.normal_fill(B, bench.DIM, 1234, 0, dev)
    x, _ = sm.sample_ode_from_base(z, method="rk4", options={"step_size": (1.0 - float(sm.sde.epsilon)) / bench.N_STEPS})
    assert np.array_equal(a, x.cpu().numpy())
