"""tools/sensor_host_check.py (CPU only): the sensor model's per-pixel kernel text (codon_amd/csrc/sensor_pixel.h with the Philox
of sensor_rng.h), built as a stand-alone program under the address and undefined-behaviour sanitizers, runs clean over the GPU
tests' cases and writes the bytes of the numpy restatement."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sensor_host_check_runs_clean():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "sensor_host_check.py")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "648 cases under -fsanitize=address,undefined" in r.stdout and "every byte equals tests/sensor_ref.py" in r.stdout
