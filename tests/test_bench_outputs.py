"""`bench.py --dump-outputs DIR`: what the last timed step computed, written as float32 / float64 .npy files within 64 MB,
the same from run to run and equal to the reference's keys; `--steps` sets the number of timed steps, and a plain run
prints a short line: the headline (the rest is `--full`).  The CPU test reads the options alone."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
ROWS = 300_000          # more than bench.DUMP_ROWS: the dump is its fixed sample of rows


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}


def test_full_and_dump_outputs_are_options():
    out = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=120, env=_env())
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def _plain_run(out_dir):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "7", "--warmup", "2", "--settle-steps", "0",
                          "--settle-seconds", "0", "--rows-per-gpu", str(ROWS), "--dump-outputs", out_dir],
                         capture_output=True, text=True, timeout=600, env=_env())
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_dump_outputs_are_the_last_steps_keys(tmp_path):
    import torch

    from lshrs_amd import LSHHasher
    from oracle import lshrs_oracle as O

    line = _plain_run(str(tmp_path / "a"))
    assert line["steps"] == 7 and line["n_gpus"] == 1 and line["unit"] == "vectors/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and abs(line["value"] - ROWS / (line["ms_per_step"] * 1e-3)) <= 1e-6 * line["value"]
    assert not {"parity_check", "rerank", "cpu_baseline", "c5", "floors", "sustained"} & set(line)
    assert len(json.dumps(line)) <= 3072 and line["roofline"]["kernel_ms_mean"] > 0      # a short line, read whole
    keys, rows = np.load(tmp_path / "a" / "keys.npy"), np.load(tmp_path / "a" / "rows.npy")
    assert keys.dtype == np.float32 and rows.dtype == np.float64
    assert keys.shape[1:] == (16, 2) and keys.shape[0] == rows.shape[0] < ROWS
    assert os.path.getsize(tmp_path / "a" / "keys.npy") + os.path.getsize(tmp_path / "a" / "rows.npy") <= 64 << 20
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < ROWS
    # same arguments, same inputs: the same outputs
    _plain_run(str(tmp_path / "b"))
    assert np.array_equal(np.load(tmp_path / "b" / "keys.npy"), keys) and np.array_equal(np.load(tmp_path / "b" / "rows.npy"), rows)
    # ... and they are the reference's keys of the rows bench.py draws for --rows-per-gpu (torch.randn on the device, seed 1000)
    x = torch.randn(ROWS, 768, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1000))
    pick = rows[:2000].astype(np.int64)
    xs = x[torch.from_numpy(pick).cuda()].cpu().numpy()
    want = O.hash_batch_literal_packed(LSHHasher(16, 16, 768, seed=42).projections, xs)
    assert np.array_equal(keys[:2000].astype(np.uint8), want)
