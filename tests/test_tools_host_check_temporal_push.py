"""tools/host_check.py temporal_push (CPU only): the workgroup bodies of the temporal stream in temporal_tile.h
-- the text the device kernels of temporal_push.hip call -- built as a stand-alone program under the address and
undefined-behaviour sanitizers, run over the GPU test's cases frame by frame and flushed, one element into larger buffers and on a
16-byte boundary, in both thread orders, with and without statistics, and write the bytes and counts of tests/temporal_ref.py on
the whole sequence.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import temporal_ref as R
from tests import temporal_stream_cases as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_temporal_push():
    n = len(S.cases())
    per_plane = sum(len(S.lengths((1, 1), w)) for w in R.WINDOWS)
    assert per_plane == 6 + 6 + 8 + 6 + 7 + 8 + 7                  # the lengths under each of temporal_ref.WINDOWS, duplicates dropped
    assert n == (len(R.PLANES) - 1) * per_plane + len(R.WINDOWS) * len(S.BIG_LENGTHS) == 309
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "temporal_push"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"temporal_push_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every byte and count equals tests/temporal_ref.py" in r.stdout, r.stdout + r.stderr
