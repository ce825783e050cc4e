"""tools/host_check.py temporal (CPU only): the workgroup body of temporal_tile.h -- the text the device kernel
calls -- built as a stand-alone program under the address and undefined-behaviour sanitizers, run over the GPU test's cases one
element into larger buffers and on a 16-byte boundary, in both thread orders, with and without statistics, and write the bytes and
counts of tests/temporal_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import temporal_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_temporal():
    n = len(R.cases())
    per_plane = sum(len(R.lengths((1, 1), w)) for w in R.WINDOWS)
    assert n == (len(R.PLANES) - 1) * per_plane + len(R.WINDOWS) * 4 + 3 == 427
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "temporal"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"temporal_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every byte and count equals tests/temporal_ref.py" in r.stdout, r.stdout + r.stderr
