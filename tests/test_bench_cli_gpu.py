"""The driver's contract for bench.py, checked on a short run: ONE JSON line on stdout with the agreed keys, the roofline object
measured live (--full), the profiled steps leaving the side streams as they were; a plain run measures the headline only and
writes the outputs of its last timed step on request."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("config", ["3", "5"])
def test_bench_prints_one_contract_line(config):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--config", config, "--steps", "3", "--warmup", "2", "--full", "--no-others",
           "--no-cpu-baseline", "--profile-steps", "1"]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["vs_baseline"] is None and d["unit"] == "images/s" and d["value"] > 0
    assert abs(d["value"] - d["config"]["crops_per_gpu"] * 1e3 / d["ms_per_step"]) <= 0.02 * d["value"]
    assert "workload" in d["config"] and d["config"]["baseline_config"] == config
    assert d["dtype"] == ("fp8" if config == "5" else "f32")
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes"):
        assert k in r, k
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    assert r["peak"] == (5000.0 if config == "5" else 416.7)       # the roof of the instruction issued: 2500 / 6 bf16 products
    if config != "5":
        assert abs(r["frac_vs_fp32_mfma"] - r["achieved"] / 157.3) < 1e-3


def _plain_run(out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", str(out)]
    env = {k: v for k, v in os.environ.items() if k != "RG_CONV_TUNE_CACHE"}
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600, env=env)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0]), {f.name: np.load(str(f)) for f in out.iterdir()}


def test_plain_run_measures_the_headline_and_dumps_its_outputs(tmp_path):
    d, files = _plain_run(tmp_path / "a")
    assert d["steps"] == 2 and d["warmup"] == 1 and d["config"]["baseline_config"] == "2" and d["dtype"] == "f32"
    assert abs(d["value"] - d["config"]["crops_per_gpu"] * 1e3 / d["ms_per_step"]) <= 0.02 * d["value"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "other_configs" not in d
    assert sum(a.nbytes for a in files.values()) <= 64 << 20
    assert {"fake.npy", "state_E.npy", "state_G.npy", "state_Di.npy", "state_Dp.npy", "loss_D_i.npy"} <= set(files)
    assert files["fake.npy"].shape == (32, 3, 256, 128)
    for name, a in files.items():
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), name
    for k, v in d["losses"].items():
        assert abs(float(files["loss_%s.npy" % k]) - v) <= 1e-5 * max(abs(v), 1.0), k
    # same arguments, same outputs: a second process runs the same recorded kernel choices on the same seeded inputs
    _, again = _plain_run(tmp_path / "b")
    assert set(again) == set(files)
    for name, a in files.items():
        assert np.array_equal(a, again[name]), name
