"""
bench.py without --full: what a plain run prints and writes (-m gpu).  It times the same steps as a --full run and
prints the headline only; every figure that takes runs of its own is left to --full (test_gpu_multirank.py checks
that line).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FULL_ONLY = ("roofline", "per_rank", "host_contention", "cpu_baseline", "configs2", "configs3_extraction_kernel", "e2e",
             "corpus_shard")


def test_plain_run_prints_the_headline_only(tmp_path):
    dump = str(tmp_path / "dump")
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--dump-outputs", dump],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    j = json.loads(lines[0])
    assert j["metric"] == "frames/sec analysis+synthesis @48kHz FFT=4096" and j["unit"] == "frames/s"
    assert j["higher_is_better"] is True and j["dtype"] == "f32" and j["n_gpus"] == 1 and j["scaling"] == "weak"
    assert j["steps"] == 5 and j["warmup"] == 2 and j["ms_per_step"] > 0
    # value = frames of the batch / time of one step
    f = j["value"] * j["ms_per_step"] * 1e-3
    assert abs(f - j["config"]["frames_per_gpu"]) < 1e-3 * f
    for k in FULL_ONLY:
        assert k not in j, k
    assert j["value_overlapped"] is None and j["value_two_launch"] is None
    assert j["config"]["overlapped"] is None and j["config"]["other_form"] is None
    assert j["config"]["ms_per_step_from_idle"] is None
    # --dump-outputs is written by a plain run as well
    d = j["dump_outputs"]
    assert d["dir"] == dump
    for name, shape in d["arrays"].items():
        a = np.load(os.path.join(dump, name + ".npy"))
        assert list(a.shape) == shape and np.all(np.isfinite(a)), name
