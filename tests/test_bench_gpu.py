"""bench.py's two kinds of run: a plain run prints the headline alone; ``--full`` adds the kernel roofline and the other
records, and the headline's timed path computes the same outputs either way."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1",
                        *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_is_the_headline_and_matches_full(tmp_path):
    plain = _bench("--dump-outputs", str(tmp_path / "plain"))
    full = _bench("--full", "--no-sub-configs", "--no-cpu-baseline", "--dump-outputs", str(tmp_path / "full"))
    for out in (plain, full):
        assert "bs=128/GPU" in out["metric"] and out["unit"] == "images/s" and out["higher_is_better"] is True
        assert out["dtype"] == "f32" and out["steps"] == 4 and out["value"] > 0 and out["ms_per_step"] > 0
    # the plain line: no records of their own, the roofline is the whole step's from the timed region alone
    assert "sub_configs" not in plain and "cpu_baseline" not in plain
    assert set(plain["roofline"]) == {"whole_step"}
    # --full: the per-launch events of the untimed cycles before the timed region name the dominant kernel
    assert full["roofline"]["kernel"].startswith("igemm<") and full["roofline"]["launches"] > 0
    names = sorted(os.listdir(tmp_path / "plain"))
    assert names == sorted(os.listdir(tmp_path / "full")) and "losses.npy" in names
    for name in names:
        a, b = np.load(tmp_path / "plain" / name), np.load(tmp_path / "full" / name)
        assert a.dtype == b.dtype and np.array_equal(a, b), name
