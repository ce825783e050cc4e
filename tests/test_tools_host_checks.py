"""tools/host_check.py (CPU only): each kernel text that also compiles for the host -- the workgroup bodies of
d4_tile.h, eval_tile.h, fill_tile.h and fill_guided_tile.h, the per-thread bodies of sensor_pixel.h and stretch_tile.h -- built
as a stand-alone program under the address and undefined-behaviour sanitizers, runs clean over the GPU tests' cases and writes
the bytes of its numpy restatement.  The counts are conditions: a driver that skips cases fails."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHECKS = {
    "d4": ("36 runs under -fsanitize=address,undefined", "every byte equals tests/d4_ref.py"),
    "sensor": ("648 cases under -fsanitize=address,undefined", "every byte equals tests/sensor_ref.py"),
    "eval": ("40 cases under -fsanitize=address,undefined", "every word and map equals tests/eval_ref.py"),
    "fill": ("144 cases under -fsanitize=address,undefined", "every output equals tests/fill_ref.py"),
    "stretch": ("504 cases under -fsanitize=address,undefined", "every output equals tests/stretch_ref.py"),
    "guided_fill": ("288 cases under -fsanitize=address,undefined", "every output equals tests/guided_fill_ref.py"),
}


@pytest.mark.parametrize("name", list(CHECKS))
def test_host_check_runs_clean(name):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), name], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    count, equals = CHECKS[name]
    assert count in r.stdout and equals in r.stdout, r.stdout + r.stderr
