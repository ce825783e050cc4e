"""tools/stretch_host_check.py (CPU only): the range normalisation's per-thread bodies (codon_amd/csrc/stretch_tile.h), built as a
stand-alone program under the address and undefined-behaviour sanitizers, run clean over the GPU tests' shapes, patterns and
formats, on and off the vector boundary, and write the ranges and planes of the numpy restatement."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stretch_host_check_runs_clean():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stretch_host_check.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "504 cases under -fsanitize=address,undefined" in r.stdout and "every output equals tests/stretch_ref.py" in r.stdout
