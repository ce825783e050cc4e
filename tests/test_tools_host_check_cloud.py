"""tools/host_check.py cloud (CPU only): the three workgroup bodies of cloud_tile.h -- the text the device
kernels call -- built as a stand-alone program under the address and undefined-behaviour sanitizers, run over the GPU test's cases
in both thread orders with the body and the normal map one byte into their buffers, and write the bytes and counts of
tests/cloud_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import cloud_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_cloud():
    n = sum(len(R.cases(s)) for s in R.SHAPES)
    assert n == (len(R.SHAPES) - 1) * len(R.PATTERNS) * len(R.FORMS) + len(R.BIG_CASES) == 396
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "cloud"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"cloud_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every byte and count equals tests/cloud_ref.py" in r.stdout, r.stdout + r.stderr
