"""tools/host_check.py clean (CPU only): the workgroup bodies of clean_tile.h -- the text the device kernels
call, the union-find's returning minimum and relaxed load spelled over the group type -- built as a stand-alone program under the
address and undefined-behaviour sanitizers, run clean over the GPU test's cases in both thread orders, with and without
statistics, and write the bytes and counts of tests/clean_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import clean_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_clean():
    n = sum(len(R.cases(s)) for s in R.SHAPES)
    assert n == len(R.SHAPES) * len(R.PATTERNS) * len(R.FORMS) == 448
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "clean"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"clean_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every output and count equals tests/clean_ref.py" in r.stdout, r.stdout + r.stderr
