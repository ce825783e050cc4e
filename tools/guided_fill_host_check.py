"""Host-side sanitizer check of the guidance-aware hole filler -- needs no GPU and loads nothing into Python:
builds tools/guided_fill_host_check.cpp (the per-thread phase bodies of codon_amd/csrc/fill_guided_tile.h, the text the device
kernels call) as a stand-alone program with the address and undefined-behaviour sanitizers, runs it workgroup by workgroup over
the GPU tests' shapes, patterns and code formats, each under all four layouts of the guidance (LAYOUTS: every load path of the
guidance reduction, the 16-byte path also with a partial last segment in the same row), the kind of guidance and the range table
following from the pattern and the layout -- and compares every output element with the numpy restatement
tests/guided_fill_ref.py.

    python tools/guided_fill_host_check.py [--cxx /opt/rocm/llvm/bin/clang++]
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
from tests import guided_fill_ref as R  # noqa: E402
from sensor_host_check import default_cxx  # noqa: E402

FORMATS = [("u8", 0, 255), ("u16", 1, 65535)]
TABLES = (10.0, 3.0, "c37")


def layouts(row):
    """(name, skew, pad) for guidance rows of `row` = w * scale bytes (a multiple of 4): the row stride is row + pad, the image
    starts skew bytes into a 16-byte aligned buffer.
      dense   as the file holds it: 16-byte segments when row % 16 == 0, else 4-byte words
      wide16  a 16-byte aligned stride wider than the row: 16-byte segments, and when row % 16 != 0 a partial last segment of
              4-byte words in the same row
      words   a stride that is a multiple of 4 but not of 16: 4-byte words throughout
      bytes   an odd start and an odd stride: bytes throughout"""
    return (("dense", 0, 0), ("wide16", 0, (-row) % 16 + 16), ("words", 0, 4 if (row + 4) % 16 else 8), ("bytes", 1, 3))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default=default_cxx(), help="a clang++ with the sanitizer runtimes")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "guided_fill_host_check")
        subprocess.run([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "guided_fill_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = lambda n: os.path.join(tmp, n)                                                        # noqa: E731
        cases = 0
        for shape in F.SHAPES:
            B, h, w = shape
            s = R.SHAPE_SCALE[shape]
            for name, fmt, top in FORMATS:
                for pi, pattern in enumerate(F.PATTERNS):
                    codes = F.case(shape, pattern, top)
                    codes.tofile(p("i"))
                    for li, (layout, skew, pad) in enumerate(layouts(w * s)):
                        kind, table = R.GUIDES[(pi + li) % 3], TABLES[(pi // 3 + li) % 3]
                        want = R.want(shape, pattern, top, s, kind, table)
                        R.guide_case(shape, s, kind).tofile(p("g"))
                        R.table_of(table).tofile(p("t"))
                        subprocess.run([exe, str(fmt), str(B), str(h), str(w), str(top), str(s), str(skew), str(pad), p("i"), p("g"),
                                        p("t"), p("o")], check=True, env=env)
                        got = np.fromfile(p("o"), dtype=codes.dtype).reshape(shape)
                        assert got.tobytes() == want.tobytes(), (shape, name, pattern, layout, kind, table)
                        cases += 1
    print(f"guided_fill_host_check: {cases} cases under -fsanitize=address,undefined over {len(F.SHAPES)} shapes x {len(FORMATS)} "
          f"formats x {len(F.PATTERNS)} patterns x 4 layouts of the guidance: no report, every output equals tests/guided_fill_ref.py")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
