"""tools/host_check.py undistort (CPU only): the workgroup body of undistort_tile.h -- the text the device
kernel calls, with the staged window, the weights and the per-thread map entries exactly sized -- and the host's tile table, built
as a stand-alone program under the address and undefined-behaviour sanitizers, run clean over the GPU test's cases in both thread
orders and write the bytes of tests/undistort_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import undistort_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_clean():
    n = sum(len(U.cases(s)) for s in U.SHAPES)
    assert n == len(U.SHAPES) * len(U.RIGS) * len(U.PATTERNS) == 120
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "undistort"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"undistort_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every output, tile table and count equals tests/undistort_ref.py" in r.stdout, r.stdout + r.stderr
