"""Host-side sanitizer check of the pull-push hole filler -- needs no GPU and loads nothing into Python: builds
tools/fill_host_check.cpp (the per-thread phase bodies of codon_amd/csrc/fill_tile.h, the text the device kernels call) as a
stand-alone program with the address and undefined-behaviour sanitizers, runs it workgroup by workgroup over the GPU tests'
shapes, patterns and formats, and compares every output element with the numpy restatement tests/fill_ref.py.

    python tools/fill_host_check.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from tests import fill_ref as F  # noqa: E402
from sensor_host_check import default_cxx  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default=default_cxx(), help="a clang++ with the sanitizer runtimes")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "fill_host_check")
        subprocess.run([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "fill_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = lambda n: os.path.join(tmp, n)                                                        # noqa: E731
        cases = 0
        for shape in F.SHAPES:
            B, h, w = shape
            for name, dtype, top, on_grid in F.FORMATS:
                tab = "-"
                if on_grid:
                    F.table(top)[:top + 1].tofile(p("t"))
                    tab = p("t")
                for pattern in F.PATTERNS:
                    codes, want = F.case(shape, pattern, top), F.want(shape, pattern, top)
                    src = F.to_grid(codes, top) if on_grid else codes
                    src.tofile(p("i"))
                    fmt = 2 if on_grid else 0 if dtype == np.uint8 else 1
                    subprocess.run([exe, str(fmt), str(B), str(h), str(w), str(top), p("i"), tab, p("o")], check=True, env=env)
                    got = np.fromfile(p("o"), dtype=src.dtype).reshape(shape)
                    ref = F.to_grid(want, top) if on_grid else want
                    assert got.tobytes() == ref.tobytes(), (shape, name, pattern)
                    cases += 1
    print(f"fill_host_check: {cases} cases under -fsanitize=address,undefined over {len(F.SHAPES)} shapes x {len(F.FORMATS)} "
          f"formats x {len(F.PATTERNS)} patterns: no report, every output equals tests/fill_ref.py")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
