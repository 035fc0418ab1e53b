"""bench.py's plain run and ``--dump-outputs``.

``dump_outputs`` writes every array as float32 ``<name>.npy`` and replaces an array over its share
of the 64 MB limit by a fixed seeded sample, the same from run to run (CPU).  On the GPU a plain
run prints the headline line without the ``--full`` measurements, times exactly ``--steps`` steps
and dumps the LLRs and channel estimates of the last one; two runs dump identical arrays.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_outputs_float32_and_seeded_sample(tmp_path, monkeypatch):
    import torch
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    big = torch.arange(5000, dtype=torch.float32).reshape(50, 100)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 2 * 4000)     # 4000 bytes per array
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big}, rank=0)
    a_small, a_big = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert a_small.dtype == np.float32 and a_small.shape == (2, 3, 4)
    np.testing.assert_array_equal(a_small, small.numpy().astype(np.float32))
    assert a_big.dtype == np.float32 and a_big.shape == (1000,)
    assert a_small.nbytes + a_big.nbytes <= 2 * 4000
    assert np.all(np.diff(a_big) >= 0) and np.isin(a_big, big.numpy()).all()   # sorted flat indices of big
    np.testing.assert_array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))
    bench.dump_outputs(str(tmp_path / "r1"), {"small": small}, rank=1)
    assert os.path.exists(tmp_path / "r1" / "small.rank1.npy")


def _plain(tmp, steps):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--prewarm-s", "0", "--batch", "4", "--dump-outputs", str(tmp)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    d = _plain(tmp_path / "a", 3)
    assert d["unit"] == "slots/s" and d["higher_is_better"] is True and d["dtype"] == "f16"
    assert d["steps"] == 3 and d["value"] > 0 and d["ms_per_step"] > 0 and d["full"] is False
    # value and ms_per_step describe the same timed region: batch slots per step
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 / 4 - 1) < 0.05
    for k in ("roofline", "cpu_baseline", "p50_latency_ms", "e2e_generate_receive_count", "kernels"):
        assert k not in d
    llr, h = np.load(tmp_path / "a" / "llr.npy"), np.load(tmp_path / "a" / "h_hat.npy")
    assert llr.dtype == h.dtype == np.float32
    assert llr.shape == (1, 4, 2, 48, 14, 4) and h.shape == (4, 2, 48, 14, 8)
    assert np.isfinite(llr).all() and np.isfinite(h).all() and np.abs(llr).max() > 1.0
    # same arguments, same inputs: a second run (another step count, so the other stream's
    # engine runs the last step) returns the same arrays
    _plain(tmp_path / "b", 2)
    np.testing.assert_array_equal(llr, np.load(tmp_path / "b" / "llr.npy"))
    np.testing.assert_array_equal(h, np.load(tmp_path / "b" / "h_hat.npy"))
