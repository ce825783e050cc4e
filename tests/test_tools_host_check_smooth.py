"""tools/host_check.py smooth (CPU only): the workgroup body of smooth_tile.h -- the text the device kernel calls
-- built as a stand-alone program under the address and undefined-behaviour sanitizers, run over the GPU test's cases with the passes
split over the launches in every way, one element into larger buffers and on a 16-byte boundary, in both thread orders, with and
without statistics, and write the bytes and counts of tests/smooth_ref.py.  The count is a condition: a driver that skips cases
fails."""
import os
import subprocess
import sys

from tests import smooth_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_smooth():
    n = len(R.cases())
    assert n == len(R.PLANES) * len(R.RADII) * len(R.PASSES) * 2 == 144
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "smooth"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"smooth_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every byte and count equals tests/smooth_ref.py" in r.stdout, r.stdout + r.stderr
