"""bench.py at the toy size, as a fresh process like the driver starts it: a plain run prints the result line without the
--full extras and reports the --steps it timed; --dump-outputs writes the last timed step's outputs, the same from run to run
up to the order of atomic sums (seeded inputs, seeded dropout); --full adds the instrumented pass's roofline object."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = {"loss", "ntokens", "grad_norm", "params_sample", "adam_exp_avg_sample", "adam_exp_avg_sq_sample"}


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "toy"] + list(extra),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_plain_run_dumps_the_same_outputs_twice(cuda, tmp_path):
    dumps = []
    for i in range(2):
        d = tmp_path / ("run%d" % i)
        out = _bench("--steps", "3", "--warmup", "1", "--dump-outputs", str(d))
        assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1
        assert out["ms_per_step"] > 0 and out["value"] > 0 and out["unit"] == "tokens/s" and out["higher_is_better"] is True
        assert out["dtype"] == "bf16" and out["roofline"] is None and out["cpu_baseline"] is None
        files = sorted(os.listdir(d))
        assert {f[:-4] for f in files} == DUMPED and all(f.endswith(".npy") for f in files)
        assert sum(os.path.getsize(d / f) for f in files) <= 64 << 20
        dumps.append({f[:-4]: np.load(d / f) for f in files})
    a, b = dumps
    for k in sorted(DUMPED):
        assert a[k].dtype in (np.float32, np.float64) and a[k].shape == b[k].shape and a[k].size > 0, k
        assert np.isfinite(a[k]).all() and np.isfinite(b[k]).all(), k
        # same inputs, same dropout masks: only the order of atomically accumulated gradient sums may differ (last bits)
        diff = float(np.abs(a[k].astype(np.float64) - b[k]).max())
        assert diff <= 1e-5 * float(np.abs(a[k]).max()), "%s differs between two runs with the same arguments: %g" % (k, diff)
    assert a["ntokens"][0] == b["ntokens"][0]
    assert a["params_sample"].size == a["adam_exp_avg_sample"].size == a["adam_exp_avg_sq_sample"].size
    assert float(a["grad_norm"][0]) > 0 and (a["adam_exp_avg_sq_sample"] >= 0).all()


@pytest.mark.gpu
def test_bench_full_adds_the_roofline(cuda):
    out = _bench("--full", "--no-cpu-baseline", "--steps", "2", "--warmup", "1")
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    assert out["roofline"] is not None and out["roofline"]["launches_per_step"] > 0
    assert out["config"]["adam_bytes_per_step"] > 0 and out["cpu_baseline"] is None
