"""tools/host_check.py mesh (CPU only): the workgroup bodies of mesh_tile.h and the two of cloud_tile.h they
follow -- the text the device kernels call -- built as a stand-alone program under the address and undefined-behaviour sanitizers,
run over the GPU test's cases in both thread orders with the face buffer one byte into its allocation, and write the bytes and
counts of tests/mesh_ref.py.  The count is a condition: a driver that skips cases fails."""
import os
import subprocess
import sys

from tests import mesh_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_check_runs_mesh():
    n = sum(len(M.cases(s)) for s in M.SHAPES)
    assert n == (len(M.SHAPES) - 1) * len(M.PATTERNS) * len(M.TOLERANCES) + len(M.BIG_CASES) == 274
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "host_check.py"), "mesh"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"mesh_host_check: {n} cases under -fsanitize=address,undefined" in r.stdout, r.stdout + r.stderr
    assert "every byte and count equals tests/mesh_ref.py" in r.stdout, r.stdout + r.stderr
