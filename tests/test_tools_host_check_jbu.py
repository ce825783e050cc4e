"""tools/host_check.py jbu (CPU only): the workgroup bodies of jbu_tile.h -- the text the device kernels call --
built as a stand-alone program under the address and undefined-behaviour sanitizers, run clean over the GPU test's cases in both
thread orders and write the bytes of tests/jbu_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import fill_ref as F
from tests import jbu_ref as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_clean():
    assert sum(len(J.cases(s)) for s in F.SHAPES) == 72
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "jbu"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "jbu_host_check: 72 cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every output equals tests/jbu_ref.py" in r.stdout, r.stdout + r.stderr
