"""The driver's bench contract: `python bench.py ...` must print ONE
JSON line with the agreed keys, value = whole-job aggregate, and run the
exact requested step count.  Run on CPU (eager path) via subprocess so
arg parsing, config loading, the measure loop and the JSON emission are
covered end-to-end."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
}


def _run(*args, device="cpu"):
    out = subprocess.run(
        [sys.executable, "bench.py", "--device", device, "--steps", "8",
         "--warmup", "2", *args],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"expected ONE JSON line, got {len(lines)}"
    return json.loads(lines[0])


def _run_bench(*extra):
    # the repeated-window measurement (under --full), probes skipped
    return _run("--full", "--min-timed-seconds", "0.05",
                "--skip-rollout-probe", "--skip-fp32-probe", *extra)


def test_bench_json_contract_default():
    d = _run_bench()
    assert REQUIRED_KEYS <= set(d)
    assert d["n_gpus"] == 1 and d["steps"] == 8 and d["warmup"] == 2
    assert d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["unit"] == "grad_steps/s" and d["data"] == "synthetic"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    # value and ms_per_step must be consistent inverses
    assert abs(d["value"] * d["ms_per_step"] / 1000.0 - 1.0) < 0.01
    cfgd = d["config"]
    for k in ("model", "global_batch", "seq_len", "parallelism"):
        assert k in cfgd
    assert cfgd["parallelism"] == "dp1"
    assert "MTSAC" in d["metric"]


def test_bench_json_contract_sac_baseline_ratio():
    d = _run_bench("--config", "sac")
    # the only derivable reference rate is the LunarLander config
    assert d["vs_baseline"] is not None
    assert abs(d["vs_baseline"] - d["value"] / 34.1) < 0.11


def test_bench_plain_run_is_one_window_and_dumps_outputs(tmp_path):
    """A plain run times exactly --steps updates (one window), runs none
    of the auxiliary probes, and --dump-outputs writes the last update's
    outputs as float32 .npy — identically from run to run."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        d = _run("--config", "sac", "--dump-outputs", str(tmp_path / name))
        assert REQUIRED_KEYS <= set(d)
        assert d["steps"] == 8 and d["timed_windows"] == 1
        assert d["env_steps_per_sec"] is None and d["fp32_value"] is None
        assert abs(d["value"] * d["ms_per_step"] / 1000.0 - 1.0) < 0.01
        files = sorted(p.name for p in (tmp_path / name).iterdir())
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    assert set(a) == set(b)
    assert set(a) == {k + ".npy" for k in (
        "metric_critic_loss", "metric_actor_loss", "metric_alpha_loss",
        "metric_entropy", "params_actor_group", "params_critic_group",
        "params_target_group", "params_alpha_group")}
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all(), k
        assert np.array_equal(a[k], b[k]), k


def test_bench_full_runs_auxiliary_measurements():
    d = _run("--config", "sac", "--full", "--min-timed-seconds", "0.05",
             "--max-windows", "3")
    assert REQUIRED_KEYS <= set(d)
    assert d["steps"] == 8 and d["timed_windows"] >= 1
    assert d["env_steps_per_sec"] > 0        # rollout probe ran


@pytest.mark.gpu
def test_bench_full_measures_fp32_rate_on_gpu():
    """--full on the GPU: the bf16 headline plus the auxiliary fp32 rate."""
    d = _run("--full", "--min-timed-seconds", "0.05", "--max-windows", "2",
             "--skip-rollout-probe", device="cuda:0")
    assert REQUIRED_KEYS <= set(d)
    assert d["dtype"] == "bf16" and d["steps"] == 8
    assert d["fp32_value"] > 0 and d["fp32_ms_per_step"] > 0
    assert d["env_steps_per_sec"] is None        # probe skipped
