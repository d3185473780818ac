"""bench.py without --full: a plain run sets up, warms up, times the steps and prints the headline line, nothing else.
The CPU baselines, the parity and rank-invariance checks, the split-precision records, the other configurations, the
streaming helpers and the committed HBM traffic belong to --full (the multi-rank rehearsals in test_gpu_full_configs.py
run it)."""
import json
import os
import socket
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]

pytestmark = pytest.mark.gpu

FULL_ONLY = ("rank_invariant", "cpu_baseline", "cpu_baseline_1thread", "parity_vs_cpu_oracle", "log_prob_rel_err",
             "log_prob_evidence", "split_precision_record", "split_precision_record_bf16x2", "extra_configs",
             "streaming_helpers")


def _line(args, env=None):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], capture_output=True, text=True, timeout=600,
                       cwd=str(ROOT), env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _assert_headline_alone(rec, steps, warmup, batch):
    assert rec["metric"] == "samples/sec (whole node), 16-dim VP-SDE 100-step RK4"
    assert rec["unit"] == "samples/s" and rec["higher_is_better"] is True and rec["dtype"] == "f32"
    assert rec["steps"] == steps and rec["warmup"] == warmup and rec["config"]["batch_per_gpu"] == batch
    assert rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(rec["n_gpus"] * batch * 1e3 / rec["ms_per_step"], rel=1e-9)
    assert rec["roofline"]["kernel_ms_avg"] > 0                       # HIP events of the timed steps themselves
    assert [k for k in FULL_ONLY if k in rec] == []
    assert rec["roofline"]["traffic"] is None and "traffic_source" not in rec["roofline"]


def test_a_plain_run_prints_the_headline_alone(built_library):
    # the default batch: the committed HBM traffic figure is for that batch, so --full would attach it here
    rec = _line(["--gpus", "1", "--steps", "1", "--warmup", "0"])
    _assert_headline_alone(rec, 1, 0, 1 << 20)
    assert rec["n_gpus"] == 1 and "per_rank" not in rec


def test_a_plain_multi_rank_run_prints_the_gathered_headline_alone(built_library):
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    rec = _line(["--gpus", "1", "--group-of-one", "--steps", "2", "--warmup", "1", "--batch", "16384"], env)
    _assert_headline_alone(rec, 2, 1, 16384)
    assert len(rec["per_rank"]["kernel_ms_avg"]) == 1 and rec["per_rank"]["allgather_ms_avg"][0] >= 0
