"""bench.py as a command on the GPU: a plain run times exactly --steps steps and does nothing beside
its headline figure; --dump-outputs writes the last timed step's contact records, equal field for field
to the oracle's for the same seeded batch (so the same from run to run); --full keeps every leg."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import gjkepa

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = 8192
FULL_ONLY = ("fp32_compute", "warm_start", "host_api", "cpu_baseline", "parity_sample", "legs", "per_rank",
             "hit_rate", "status_counts", "epa_iters_mean")


def _bench(tmp_path, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--pairs-per-gpu", str(PAIRS), *extra]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=110, cwd=str(tmp_path))
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path, orc):
    import bench
    r = _bench(tmp_path, "--dump-outputs", str(tmp_path / "a"))
    assert r["metric"] == bench.METRIC and r["unit"] == "M queries/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f64" and r["steps"] == 3 and r["warmup"] == 1 and r["n_gpus"] == 1
    assert r["ms_per_step"] > 0 and r["value"] > 0
    # value = pairs per step / ms_per_step; the line rounds them to 3 and 4 decimals
    assert abs(r["value"] - PAIRS / (r["ms_per_step"] * 1e-3) / 1e6) <= r["value"] * 0.5e-4 / r["ms_per_step"] + 1e-3
    assert r["dominant_kernel"] is None and not [k for k in FULL_ONLY if k in r], sorted(r)
    assert r["outputs"]["records"] == PAIRS == r["outputs"]["of"]
    # the records are the oracle's for the same batch, field for field
    pool = gjkepa.synth_pairs(bench.SEED, PAIRS, 32, 32, 2.5, dtype=np.float32)
    ref = orc.gjkepa_batch(pool, 2, 1.0)
    assert (np.load(tmp_path / "a" / "pair_index.npy") == np.arange(PAIRS)).all()
    for name in bench.DUMP_FIELDS:
        a = np.load(tmp_path / "a" / (name + ".npy"))
        assert a.dtype == np.float64 and len(a) == PAIRS, name
        assert a.tobytes() == np.ascontiguousarray(ref[name]).astype(np.float64).tobytes(), name


def test_full_run_keeps_every_leg(tmp_path):
    r = _bench(tmp_path, "--full", "--cpu-sample", "2048", "--legs", "none")
    for k in ("fp32_compute", "warm_start", "host_api", "cpu_baseline", "hit_rate", "status_counts"):
        assert k in r, k
    assert r["parity_sample"]["all_equal"] and r["parity_sample"]["pairs"] == 2048
    assert r["dominant_kernel"] is not None and r["dominant_kernel"]["timing"].startswith("separate")
