"""Host-side sanitizer check of the D4 self-ensemble kernels -- needs no GPU and loads nothing into Python:
builds tools/d4_host_check.cpp (the per-thread bodies of codon_amd/csrc/d4_tile.h, the text the device kernels call) as a
stand-alone program with the address and undefined-behaviour sanitizers, runs it thread by thread over the GPU tests' shapes
and all three dtypes, and compares every byte it writes with the numpy restatement tests/d4_ref.py.

    python tools/d4_host_check.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import d4_ref as D  # noqa: E402

DT_CODE = {"f32": 0, "bf16": 1, "f16": 2}          # codon_dtype


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default=os.environ.get("CXX", "clang++"), help="a clang++ (the bodies use _Float16 and __builtin_bit_cast)")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "d4_host_check")
        subprocess.run([a.cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", os.path.join(ROOT, "tools", "d4_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = lambda n: os.path.join(tmp, n)                                                        # noqa: E731
        cases = 0
        for shape in D.SHAPES:
            B, H, W = shape
            for dt in ("f32", "f16", "bf16"):
                x, y = D.random_bits(shape, dt, 1), D.random_bits(shape, dt, 2)
                x.tofile(p("x")), y.tofile(p("y"))
                for two in (True, False):
                    subprocess.run([exe, "views", str(x.itemsize), str(B), str(H), str(W), p("x"), p("y") if two else "-", p("v")],
                                   check=True, env=env)
                    for src, names in ((x, ("v.up0", "v.tp0")),) + (((y, ("v.up1", "v.tp1")),) if two else ()):
                        for ref, n in zip(D.views(src), names):
                            got = np.fromfile(p(n), dtype=src.dtype).reshape(ref.shape)
                            assert np.array_equal(got, ref), ("views", shape, dt, two, n)
                            os.remove(p(n))
                    cases += 1
                up, tr = D.merge_values(4 * B, H, W, dt, 3), D.merge_values(4 * B, W, H, dt, 4)
                up.tofile(p("u")), tr.tofile(p("t"))
                subprocess.run([exe, "merge", str(DT_CODE[dt]), str(B), str(H), str(W), p("u"), p("t"), p("o")], check=True, env=env)
                ref = D.merge(D.upcast(up, dt), D.upcast(tr, dt))
                got = np.fromfile(p("o"), dtype=np.float32).reshape(ref.shape)
                assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), ("merge", shape, dt)
                cases += 1
    print(f"d4_host_check: {cases} runs under -fsanitize=address,undefined over {len(D.SHAPES)} shapes x 3 dtypes: "
          "no report, every byte equals tests/d4_ref.py")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
