"""tools/host_check.py register (CPU only): the workgroup bodies of register_tile.h -- the text the device
kernels call, the atomic minimum and add spelled over the group type -- built as a stand-alone program under the address and
undefined-behaviour sanitizers, run clean over the GPU test's cases in both thread orders and write the bytes of
tests/register_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import register_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_clean():
    n = sum(len(G.cases(s)) for s in G.SHAPES)
    assert n == len(G.SHAPES) * len(G.PATTERNS) * len(G.CALIBS) == 120
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "register"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"register_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every output equals tests/register_ref.py" in r.stdout, r.stdout + r.stderr
