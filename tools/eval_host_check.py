"""Host-side sanitizer check of the depth evaluation kernel -- needs no GPU and loads nothing into Python:
builds tools/eval_host_check.cpp (the per-thread phase bodies of codon_amd/csrc/eval_tile.h, the text the device kernel calls)
as a stand-alone program with the address and undefined-behaviour sanitizers, runs it thread by thread over the GPU tests' shapes,
both code widths, every radius and the edge-off / two-threshold form, and compares the sixteen words and both maps it writes
with the numpy restatement tests/eval_ref.py.

    python tools/eval_host_check.py [--cxx /opt/rocm/llvm/bin/clang++]
"""
import argparse
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
from tests import eval_ref as E  # noqa: E402
from sensor_host_check import default_cxx  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cxx", default=default_cxx(), help="a clang++ with the sanitizer runtimes")
    a = ap.parse_args(argv)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "eval_host_check")
        subprocess.run([a.cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(ROOT, "tools", "eval_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        p = lambda n: os.path.join(tmp, n)                                                        # noqa: E731
        cases = 0
        for shape in E.SHAPES:
            B, H, W = shape
            for bits in (8, 16):
                label, out = E.case(shape, bits)
                label.tofile(p("l")), out.tofile(p("o"))
                full = E.PARAMS[bits]
                forms = [dict(full, edge_radius=r) for r in E.RADII] + [{"thresholds": full["thresholds"][:2], "edge_threshold": None}]
                for kw in forms:
                    thr, T = kw["thresholds"], kw["edge_threshold"]
                    args = [bits, B, H, W, label.shape[1], label.shape[2], len(thr), *(list(thr) + [0] * 4)[:4],
                            0 if T is None else 1, 0 if T is None else T, kw.get("edge_radius", 0)]
                    subprocess.run([exe, *(str(v) for v in args), p("l"), p("o"), p("r")], check=True, env=env)
                    words, err, reg = E.depth_errors_batch(label, out, **kw)
                    assert np.array_equal(np.fromfile(p("r.acc"), dtype=np.uint64).reshape(B, E.WORDS), words), ("words", shape, bits, kw)
                    assert np.array_equal(np.fromfile(p("r.err"), dtype=out.dtype).reshape(out.shape), err), ("error map", shape, bits, kw)
                    assert np.array_equal(np.fromfile(p("r.reg"), dtype=np.uint8).reshape(out.shape), reg), ("region map", shape, bits, kw)
                    cases += 1
    print(f"eval_host_check: {cases} cases under -fsanitize=address,undefined over {len(E.SHAPES)} shapes x 2 code widths: "
          "no report, every word and map equals tests/eval_ref.py")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
