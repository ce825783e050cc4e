"""tools/host_check.py normal_errors (CPU only): the workgroup body of normal_tile.h -- the text the device
kernel calls -- built as a stand-alone program under the address and undefined-behaviour sanitizers, run clean over the GPU test's
cases in both thread orders and write the words and maps of tests/normal_errors_ref.py; the per-pair index function over pairs no
scene reaches.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import normal_errors_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_clean():
    assert sum(len(N.cases(s)) for s in N.SHAPES) == 336
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "normal_errors"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "normal_errors_host_check: 336 cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every word and map equals tests/normal_errors_ref.py" in r.stdout, r.stdout + r.stderr
