"""Host-side sanitizer check of the per-image range normalisation -- needs no GPU and loads nothing into Python:
builds tools/stretch_host_check.cpp (the per-thread bodies of codon_amd/csrc/stretch_tile.h, the text the device kernels call) as
a stand-alone program with the address and undefined-behaviour sanitizers, runs it workgroup by workgroup over the GPU tests'
shapes, patterns and formats -- every case with the planes on a vector boundary and one element off it -- and compares the
ranges, the stretched planes and the planes stretched and mapped back with the numpy restatement tests/stretch_ref.py.

    python tools/stretch_host_check.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from tests import stretch_ref as S  # noqa: E402
from sensor_host_check import default_cxx  # noqa: E402

SKEWS = (0, 1)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default=default_cxx(), help="a clang++ with the sanitizer runtimes")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "stretch_host_check")
        subprocess.run([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "stretch_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = lambda n: os.path.join(tmp, n)                                                        # noqa: E731
        cases = 0
        for shape in S.SHAPES:
            B, h, w = shape
            for name, dtype, top in S.FORMATS:
                for pattern in S.PATTERNS:
                    codes = S.case(shape, pattern, top)
                    want, rng = S.want(shape, pattern, top)
                    back = S.unstretch_batch(want, rng, top)
                    codes.tofile(p("i"))
                    for skew in SKEWS:
                        subprocess.run([exe, "0" if dtype == np.uint8 else "1", str(B), str(h * w), str(top), str(skew), p("i"),
                                        p("r"), p("s"), p("b")], check=True, env=env)
                        what = (shape, name, pattern, skew)
                        assert np.fromfile(p("r"), dtype=np.int32).tobytes() == rng.tobytes(), what
                        assert np.fromfile(p("s"), dtype=dtype).tobytes() == want.tobytes(), what
                        assert np.fromfile(p("b"), dtype=dtype).tobytes() == back.tobytes(), what
                        cases += 1
    print(f"stretch_host_check: {cases} cases under -fsanitize=address,undefined over {len(S.SHAPES)} shapes x {len(S.FORMATS)} "
          f"formats x {len(S.PATTERNS)} patterns x {len(SKEWS)} alignments: no report, every output equals tests/stretch_ref.py")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
