"""Host-side sanitizer check of the sensor model's kernel -- needs no GPU and loads nothing into Python: builds
tools/sensor_host_check.cpp (the per-pixel body of codon_amd/csrc/sensor_pixel.h with the Philox of sensor_rng.h, the text the
device kernel calls) as a stand-alone program with the address and undefined-behaviour sanitizers, runs it pixel by pixel over
the GPU tests' cases (tests/sensor_ref.cases: every size, batch, level count, mode, parameter set and hole pattern) and
compares every byte it writes with the numpy restatement tests/sensor_ref.py.

    python tools/sensor_host_check.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import shutil
import struct
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import resample_masked_ref as M  # noqa: E402
from tests import sensor_ref as S  # noqa: E402


def default_cxx():
    """$CXX, a clang++ on the PATH, or the one ROCm ships next to hipcc."""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    return os.environ.get("CXX") or shutil.which("clang++") or (rocm if os.path.exists(rocm) else "clang++")


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default=default_cxx(), help="a clang++ with the sanitizer runtimes")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "sensor_host_check")
        subprocess.run([a.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "sensor_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        S.gauss_table().tofile(os.path.join(tmp, "gauss.bin"))
        for levels in S.LEVELS:
            np.ascontiguousarray(M.tables(8 if levels == 255 else 16, levels)[1][:levels + 1]).tofile(os.path.join(tmp, f"lut{levels}.bin"))
        total = 0
        for B in S.BATCHES:
            for p in S.SIZES:
                want = []
                with open(os.path.join(tmp, "cases.bin"), "wb") as f:
                    for c in S.cases(B, p):
                        lr = S.input_map(B, p, c["kind"], c["levels"], c["masked"], c["seed"])
                        f.write(struct.pack("<4i4I3fI2Q", B, p, c["masked"], c["levels"], S.KEY[0], S.KEY[1], c["step"], c["first"],
                                            c["sigma"], c["quad"], c["edge_thr"], 0, S.threshold(c["p_drop"]), S.threshold(c["p_edge"])))
                        f.write(lr.tobytes())
                        want.append((c["name"], S.run_case(c, lr)))
                subprocess.run([exe, tmp], check=True, env=env, stdout=subprocess.DEVNULL)
                got = np.fromfile(os.path.join(tmp, "out.bin"), dtype=np.uint32)
                assert got.size == len(want) * B * p * p, (B, p, got.size)
                for k, (name, ref) in enumerate(want):
                    g = got[k * ref.size:(k + 1) * ref.size].reshape(ref.shape)
                    assert np.array_equal(g, ref.view(np.uint32)), name
                total += len(want)
    print(f"sensor_host_check: {total} cases under -fsanitize=address,undefined over {len(S.BATCHES)} batches x {len(S.SIZES)} "
          "sizes: no report, every byte equals tests/sensor_ref.py")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
