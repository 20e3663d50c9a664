"""bench.py's command line: a plain run times the headline and nothing else, --full adds the other measurements, --dump-outputs
writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_bench_options_default_to_a_plain_run():
    sys.path.insert(0, ROOT) if ROOT not in sys.path else None
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--full", "--dump-outputs", "out", "--no-sweep"])
    assert a.full is True and a.dump_outputs == "out" and a.no_sweep is True


@pytest.mark.gpu
def test_plain_bench_run_times_the_headline_and_dumps_its_outputs(tmp_path):
    out = tmp_path / "outputs"
    env = dict(os.environ, BANET_BENCH_DETAIL_DIR=str(tmp_path))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads(r.stdout.strip().split("\n")[-1])
    assert rec["steps"] == 2 and rec["warmup"] == 1 and rec["ms_per_step"] > 0 and rec["value"] > 0
    assert rec["unit"] == "LM iterations/s" and rec["higher_is_better"] is True and rec["dtype"].startswith("f32")
    for k in ("parity", "cpu_baseline", "sweep", "backward", "value_exact_syrk"):       # --full only
        assert k not in rec, k
    B, K, L = 32, 128, 5
    arrays = {p[:-4]: np.load(str(out / p)) for p in os.listdir(str(out))}
    assert set(arrays) == {"records", "R", "T", "W", "lambda", "delta", "ratio", "iters_per_level"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert arrays["records"].shape == (B, 12 + K + L) and arrays["W"].shape == (B, K, 1)
    # the records are the state the solver returned, packed: R | T | W | iterations per level
    assert np.array_equal(arrays["records"][:, :9], arrays["R"].reshape(B, 9))
    assert np.array_equal(arrays["records"][:, 9:12], arrays["T"].reshape(B, 3))
    assert np.array_equal(arrays["records"][:, 12:12 + K], arrays["W"].reshape(B, K))
    assert (arrays["iters_per_level"] == 10).all()
