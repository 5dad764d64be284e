"""bench.py without --full: the headline line only (no CPU baseline, no kernel profile), --steps timed steps, and
--dump-outputs writing what two steps of the timed path return from the seeded initial state, as float32 / float64
.npy files, 64 MB at most, the same in every run up to the rounding of the backward's float atomics."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "4",
           "--batch", "2", "--height", "64", "--width", "128", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(str(out / f)) for f in sorted(os.listdir(str(out)))}


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_reproducible_outputs(dev, tmp_path):
    d, arrays = _bench(tmp_path / "a")
    assert d["steps"] == 3 and d["warmup"] == 4 and d["unit"] == "samples/s" and d["higher_is_better"] is True
    assert d["dtype"] == "bf16" and d["ms_per_step"] > 0
    assert abs(d["value"] - 2 * 3 / (d["ms_per_step"] * 3e-3)) < 0.02 * d["value"]
    assert d["config"]["hipgraph_replays"] == 3                 # the timed steps are replays of the captured step
    assert "cpu_baseline" not in d and d["roofline"] is None and d["kernels"] == {} and d["ms_per_step_200"] is None
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values()), {k: a.dtype for k, a in arrays.items()}
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    names = {"loss", "loss_dict.total_loss", "loss_dict.loss_0", "loss_dict.smooth_loss_0"}
    assert {"step1." + k for k in names} | {"step1.grad_norm", "step2.loss"} <= set(arrays), sorted(arrays)
    assert all(np.isfinite(a).all() for a in arrays.values())
    assert float(arrays["step1.loss"]) == float(arrays["step1.loss_dict.total_loss"])
    assert float(arrays["step1.grad_norm"]) > 0, arrays["step1.grad_norm"]
    # same arguments, same inputs (seeded batches, seeded initial state): step 1 is a forward from identical inputs, bit
    # for bit; what depends on a backward agrees up to the rounding of its float atomics
    _, again = _bench(tmp_path / "b")
    assert sorted(again) == sorted(arrays)
    for k, a in arrays.items():
        if k.startswith("step1.") and k != "step1.grad_norm":
            assert np.array_equal(a, again[k]), (k, a, again[k])
        else:
            np.testing.assert_allclose(again[k], a, rtol=1e-5, atol=0, err_msg=k)
