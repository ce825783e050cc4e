"""tools/eval_host_check.py (CPU only): the depth evaluation kernel's per-thread phase bodies (codon_amd/csrc/eval_tile.h), built
as a stand-alone program under the address and undefined-behaviour sanitizers, run clean over the GPU tests' cases and write the
words and maps of the numpy restatement."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_host_check_runs_clean():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "eval_host_check.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "40 cases under -fsanitize=address,undefined" in r.stdout and "every word and map equals tests/eval_ref.py" in r.stdout
