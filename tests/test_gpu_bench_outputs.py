"""GPU: a plain bench.py run (no --full) and its --dump-outputs files. The line keeps the headline
fields and leaves every figure that needs a run of its own null; the dumped arrays are float32,
within 64 MB, and identical from run to run with the same arguments (seeded inputs,
deterministic kernels), so two builds can be compared output for output."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, WARMUP = 6, 3
NAMES = ["W_sample", "W_updated", "grad_scale", "table_absmax", "table_scale", "y"]


def _bench(out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup",
           str(WARMUP), "--config", "kaggle", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("bench_outputs")
    return [(_bench(d / k), d / k) for k in ("a", "b")]


def test_plain_line_has_headline_only(runs):
    line, _ = runs[0]
    assert line["full"] is False and line["steps"] == STEPS and line["warmup"] == WARMUP
    assert line["value"] > 0 and line["unit"] == "samples/s" and line["higher_is_better"] is True
    assert line["ms_per_step"] > 0 and line["device_errors"] == 0
    # value is samples per second of the timed steps: global batch / step time
    assert line["value"] == pytest.approx(line["config"]["global_batch"] / (line["us_per_step"] * 1e-6), rel=1e-2)
    for k in ("roofline", "step_roofline", "kernels_ms", "int4_gather", "mlp_grad_exchange", "cpu_baseline",
              "cpu_baseline_oracle_c", "replicas_bit_identical"):
        assert line[k] is None, k
    assert line["outputs_dumped"] == NAMES


def test_dumped_outputs_float32_bounded_and_sane(runs):
    line, d = runs[0]
    assert sorted(os.listdir(d)) == [n + ".npy" for n in NAMES]
    arrs = {n: np.load(d / (n + ".npy")) for n in NAMES}
    assert all(a.dtype == np.float32 for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    T, B, D = line["config"]["tables"], line["config"]["batch_per_gpu"], line["config"]["emb_dim"]
    assert arrs["y"].shape == (T * B, D) and arrs["W_updated"].shape == (T * B, D)
    assert arrs["table_scale"].shape == (T,) and arrs["grad_scale"].shape == (T,)
    assert all(np.isfinite(a).all() for a in arrs.values())
    # INT4 fake-quant output: every element is an integer in [-8, 7] times its table's scale
    q = arrs["y"].reshape(T, B, D) / arrs["table_scale"].reshape(T, 1, 1)
    assert np.abs(q - np.round(q)).max() < 1e-3 and q.min() >= -8.001 and q.max() <= 7.001
    assert np.abs(arrs["W_updated"]).max() <= arrs["table_absmax"].max()


def test_dumped_outputs_identical_between_runs(runs):
    (_, da), (_, db) = runs
    for n in NAMES:
        assert np.array_equal(np.load(da / (n + ".npy")), np.load(db / (n + ".npy"))), n
