"""bench.py's plain run and --dump-outputs: what the timed path returned in its last step, as .npy files, from
inputs that are the same from run to run (so that two builds can be compared output for output)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

NAMES = ("dx", "dy", "dz", "dw")


def _load(directory):
    return {name: np.load(os.path.join(directory, name + ".npy")) for name in NAMES + ("residual",)}


def test_dump_outputs_whole_blocks_below_the_limit(tmp_path):
    d = [np.arange(10.0), np.ones(3, dtype=np.float32), np.zeros(0), -np.arange(5.0)]
    bench.dump_outputs(str(tmp_path), d, 3e-14)
    got = _load(str(tmp_path))
    for name, ref in zip(NAMES, d):
        assert got[name].dtype == np.float64 and np.array_equal(got[name], ref)
    assert got["residual"].tolist() == [3e-14]


def test_dump_outputs_fixed_sample_above_the_limit(tmp_path):
    n = bench.DUMP_LIMIT_BYTES // 8
    d = [np.arange(float(n)), np.arange(float(n // 2)), np.arange(7.0), np.arange(7.0)]
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), d, 1.0)
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= bench.DUMP_LIMIT_BYTES
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    for name in NAMES:
        assert np.array_equal(a[name], b[name])                      # the same sample every time
        assert np.all(np.diff(a[name]) > 0)                          # sorted entries of the block, no repeats
    assert a["dx"].size > a["dy"].size > 0 and a["dz"].size <= 7


def test_steps_must_be_positive():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True,
                         timeout=120, cwd=ROOT)
    assert out.returncode == 2 and "--steps" in out.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(tmp_path):
    """A plain run at a small C4 size prints the headline line alone (nothing of --full), and two runs with the same
    arguments dump the same outputs: the solution blocks of the system the line describes and its residual."""
    recs = []
    for sub in ("a", "b"):
        cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--stages", "6", "--nx", "1024",
               "--steps", "2", "--warmup", "1", "--dump-outputs", str(tmp_path / sub)]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, lines
        recs.append(json.loads(lines[0]))
    rec = recs[0]
    assert rec["steps"] == 2 and rec["ms_per_step"] > 0 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) <= 1e-9 * rec["value"]
    for key in ("roofline", "kernels", "cpu_baseline", "ip_iterations_c4", "value_with_host_vectors"):
        assert key not in rec
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    cfg = rec["config"]
    assert [a[k].size for k in NAMES] == [cfg["n"], cfg["me"], cfg["m"], cfg["m"]]
    assert a["residual"][0] == rec["residual"] <= 1e-10
    assert all(np.isfinite(a[k]).all() for k in NAMES) and np.abs(a["dx"]).max() > 0
    for k in NAMES:  # (same inputs; the products may sum in another order from run to run)
        assert np.abs(a[k] - b[k]).max() <= 1e-10 * max(np.abs(b[k]).max(), 1e-300), k
