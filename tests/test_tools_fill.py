"""tools/fill_host_check.py (CPU only): the hole filler's per-thread phase bodies (codon_amd/csrc/fill_tile.h), built as a
stand-alone program under the address and undefined-behaviour sanitizers, run clean over the GPU tests' shapes, patterns and
formats and write the planes of the numpy restatement."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fill_host_check_runs_clean():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "fill_host_check.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "144 cases under -fsanitize=address,undefined" in r.stdout and "every output equals tests/fill_ref.py" in r.stdout
