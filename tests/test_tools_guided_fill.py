"""tools/guided_fill_host_check.py (CPU only): the guided hole filler's per-thread phase bodies
(codon_amd/csrc/fill_guided_tile.h), built as a stand-alone program under the address and undefined-behaviour sanitizers, run
clean over the GPU tests' shapes, patterns and code formats under four layouts of the guidance and write the planes of the numpy
restatement."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_guided_fill_host_check_runs_clean():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "guided_fill_host_check.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "288 cases under -fsanitize=address,undefined" in r.stdout and "every output equals tests/guided_fill_ref.py" in r.stdout
