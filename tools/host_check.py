"""Host-side sanitizer checks of the kernels whose text also compiles for the host -- need no GPU and load nothing
into Python.  Each check builds tools/NAME_host_check.cpp -- a stand-alone program around the workgroup bodies (d4, eval, fill,
guided_fill, jbu, register, clean, undistort, cloud, mesh, normal_errors, temporal, temporal_push, smooth) or per-thread bodies (sensor, stretch) of a header under codon_amd/csrc/, the text the device kernels call -- with the
address and undefined-behaviour sanitizers, runs it over the GPU tests' cases and compares every byte it writes with the numpy
restatement tests/NAME_ref.py.  The programs that run workgroup bodies run every case with both thread orders themselves.

    python tools/host_check.py NAME|all [--cxx /opt/rocm/llvm/bin/clang++]
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
from tests import clean_ref as K  # noqa: E402
from tests import cloud_ref as Q  # noqa: E402
from tests import d4_ref as D  # noqa: E402
from tests import eval_ref as E  # noqa: E402
from tests import fill_ref as F  # noqa: E402
from tests import guided_fill_ref as R  # noqa: E402
from tests import jbu_ref as J  # noqa: E402
from tests import mesh_ref as H  # noqa: E402
from tests import normal_errors_ref as N  # noqa: E402
from tests import register_ref as G  # noqa: E402
from tests import resample_masked_ref as M  # noqa: E402
from tests import sensor_ref as S  # noqa: E402
from tests import smooth_ref as Y  # noqa: E402
from tests import stretch_ref as T  # noqa: E402
from tests import temporal_ref as V  # noqa: E402
from tests import temporal_stream_cases as W  # noqa: E402
from tests import undistort_ref as U  # noqa: E402

FLAGS = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def default_cxx():
    """$CXX, a clang++ on the PATH, or the one ROCm ships next to hipcc."""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang++")
    return os.environ.get("CXX") or shutil.which("clang++") or (rocm if os.path.exists(rocm) else "clang++")


# A check is a function (run, p) -> (count, "what was covered: no report, what equals what"): run(*args) runs the program, which
# must exit 0; p(name) is a path in the temporary directory.

def d4(run, p):
    code = {"f32": 0, "bf16": 1, "f16": 2}                                                        # codon_dtype
    runs = 0
    for shape in D.SHAPES:
        B, H, W = shape
        for dt in ("f32", "f16", "bf16"):
            x, y = D.random_bits(shape, dt, 1), D.random_bits(shape, dt, 2)
            x.tofile(p("x")), y.tofile(p("y"))
            for two in (True, False):
                run("views", x.itemsize, B, H, W, p("x"), p("y") if two else "-", p("v"))
                for src, names in ((x, ("v.up0", "v.tp0")),) + (((y, ("v.up1", "v.tp1")),) if two else ()):
                    for ref, n in zip(D.views(src), names):
                        got = np.fromfile(p(n), dtype=src.dtype).reshape(ref.shape)
                        assert np.array_equal(got, ref), ("views", shape, dt, two, n)
                        os.remove(p(n))
                runs += 1
            up, tr = D.merge_values(4 * B, H, W, dt, 3), D.merge_values(4 * B, W, H, dt, 4)
            up.tofile(p("u")), tr.tofile(p("t"))
            run("merge", code[dt], B, H, W, p("u"), p("t"), p("o"))
            ref = D.merge(D.upcast(up, dt), D.upcast(tr, dt))
            got = np.fromfile(p("o"), dtype=np.float32).reshape(ref.shape)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), ("merge", shape, dt)
            runs += 1
    return runs, f"over {len(D.SHAPES)} shapes x 3 dtypes: no report, every byte equals tests/d4_ref.py"


def sensor(run, p):
    S.gauss_table().tofile(p("gauss.bin"))
    for levels in S.LEVELS:
        np.ascontiguousarray(M.tables(8 if levels == 255 else 16, levels)[1][:levels + 1]).tofile(p(f"lut{levels}.bin"))
    total = 0
    for B in S.BATCHES:
        for size in S.SIZES:
            want = []
            with open(p("cases.bin"), "wb") as f:
                for c in S.cases(B, size):
                    lr = S.input_map(B, size, c["kind"], c["levels"], c["masked"], c["seed"])
                    f.write(struct.pack("<4i4I3fI2Q", B, size, c["masked"], c["levels"], S.KEY[0], S.KEY[1], c["step"], c["first"],
                                        c["sigma"], c["quad"], c["edge_thr"], 0, S.threshold(c["p_drop"]), S.threshold(c["p_edge"])))
                    f.write(lr.tobytes())
                    want.append((c["name"], S.run_case(c, lr)))
            run(os.path.dirname(p("")))
            got = np.fromfile(p("out.bin"), dtype=np.uint32)
            assert got.size == len(want) * B * size * size, (B, size, got.size)
            for k, (name, ref) in enumerate(want):
                assert np.array_equal(got[k * ref.size:(k + 1) * ref.size].reshape(ref.shape), ref.view(np.uint32)), name
            total += len(want)
    return total, f"over {len(S.BATCHES)} batches x {len(S.SIZES)} sizes: no report, every byte equals tests/sensor_ref.py"


def eval_(run, p):
    cases = 0
    for shape in E.SHAPES:
        B, H, W = shape
        for bits in (8, 16):
            label, out = E.case(shape, bits)
            label.tofile(p("l")), out.tofile(p("o"))
            full = E.PARAMS[bits]
            forms = [dict(full, edge_radius=r) for r in E.RADII] + [{"thresholds": full["thresholds"][:2], "edge_threshold": None}]
            for kw in forms:
                thr, thr_e = kw["thresholds"], kw["edge_threshold"]
                run(bits, B, H, W, label.shape[1], label.shape[2], len(thr), *(list(thr) + [0] * 4)[:4],
                    0 if thr_e is None else 1, 0 if thr_e is None else thr_e, kw.get("edge_radius", 0), p("l"), p("o"), p("r"))
                words, err, reg = E.depth_errors_batch(label, out, **kw)
                assert np.array_equal(np.fromfile(p("r.acc"), dtype=np.uint64).reshape(B, E.WORDS), words), ("words", shape, bits, kw)
                assert np.array_equal(np.fromfile(p("r.err"), dtype=out.dtype).reshape(out.shape), err), ("error map", shape, bits, kw)
                assert np.array_equal(np.fromfile(p("r.reg"), dtype=np.uint8).reshape(out.shape), reg), ("region map", shape, bits, kw)
                cases += 1
    return cases, f"over {len(E.SHAPES)} shapes x 2 code widths: no report, every word and map equals tests/eval_ref.py"


def fill(run, p):
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
                run(2 if on_grid else 0 if dtype == np.uint8 else 1, B, h, w, top, p("i"), tab, p("o"))
                got = np.fromfile(p("o"), dtype=src.dtype).reshape(shape)
                ref = F.to_grid(want, top) if on_grid else want
                assert got.tobytes() == ref.tobytes(), (shape, name, pattern)
                cases += 1
    return cases, (f"over {len(F.SHAPES)} shapes x {len(F.FORMATS)} formats x {len(F.PATTERNS)} patterns: no report, "
                   "every output equals tests/fill_ref.py")


def stretch(run, p):
    skews = (0, 1)      # the planes on a vector boundary and one element off it
    cases = 0
    for shape in T.SHAPES:
        B, h, w = shape
        for name, dtype, top in T.FORMATS:
            for pattern in T.PATTERNS:
                codes = T.case(shape, pattern, top)
                want, rng = T.want(shape, pattern, top)
                back = T.unstretch_batch(want, rng, top)
                codes.tofile(p("i"))
                for skew in skews:
                    run(0 if dtype == np.uint8 else 1, B, h * w, top, skew, p("i"), p("r"), p("s"), p("b"))
                    what = (shape, name, pattern, skew)
                    assert np.fromfile(p("r"), dtype=np.int32).tobytes() == rng.tobytes(), what
                    assert np.fromfile(p("s"), dtype=dtype).tobytes() == want.tobytes(), what
                    assert np.fromfile(p("b"), dtype=dtype).tobytes() == back.tobytes(), what
                    cases += 1
    return cases, (f"over {len(T.SHAPES)} shapes x {len(T.FORMATS)} formats x {len(T.PATTERNS)} patterns x {len(skews)} "
                   "alignments: no report, every output equals tests/stretch_ref.py")


def guided_layouts(row):
    """(name, skew, pad) for guidance rows of `row` = w * scale bytes (a multiple of 4): the row stride is row + pad, the image
    starts skew bytes into a 16-byte aligned buffer.
      dense   as the file holds it: 16-byte segments when row % 16 == 0, else 4-byte words
      wide16  a 16-byte aligned stride wider than the row: 16-byte segments, and when row % 16 != 0 a partial last segment of
              4-byte words in the same row
      words   a stride that is a multiple of 4 but not of 16: 4-byte words throughout
      bytes   an odd start and an odd stride: bytes throughout"""
    return (("dense", 0, 0), ("wide16", 0, (-row) % 16 + 16), ("words", 0, 4 if (row + 4) % 16 else 8), ("bytes", 1, 3))


def guided_fill(run, p):
    """Every load path of the guidance reduction; the kind of guidance and the range table follow from pattern and layout."""
    formats, tables = [("u8", 0, 255), ("u16", 1, 65535)], (10.0, 3.0, "c37")
    cases = 0
    for shape in F.SHAPES:
        B, h, w = shape
        s = R.SHAPE_SCALE[shape]
        for name, fmt, top in formats:
            for pi, pattern in enumerate(F.PATTERNS):
                codes = F.case(shape, pattern, top)
                codes.tofile(p("i"))
                for li, (layout, skew, pad) in enumerate(guided_layouts(w * s)):
                    kind, table = R.GUIDES[(pi + li) % 3], tables[(pi // 3 + li) % 3]
                    want = R.want(shape, pattern, top, s, kind, table)
                    R.guide_case(shape, s, kind).tofile(p("g"))
                    R.table_of(table).tofile(p("t"))
                    run(fmt, B, h, w, top, s, skew, pad, p("i"), p("g"), p("t"), p("o"))
                    got = np.fromfile(p("o"), dtype=codes.dtype).reshape(shape)
                    assert got.tobytes() == want.tobytes(), (shape, name, pattern, layout, kind, table)
                    cases += 1
    return cases, (f"over {len(F.SHAPES)} shapes x {len(formats)} formats x {len(F.PATTERNS)} patterns x 4 layouts of the guidance: "
                   "no report, every output equals tests/guided_fill_ref.py")


def jbu(run, p):
    """The GPU test's cases (jbu_ref.cases), each with the layout of the guidance its row names: both load paths of a run."""
    cases = 0
    for shape in F.SHAPES:
        B, h, w = shape
        s = R.SHAPE_SCALE[shape]
        for name, top, pattern, kind, sigma_s, li in J.cases(shape):
            layout, skew, pad = guided_layouts(w * s)[li]
            codes = F.case(shape, pattern, top)
            codes.tofile(p("i"))
            R.guide_case(shape, s, kind).tofile(p("g"))
            R.table_of(10.0).tofile(p("t"))
            J.spatial_table(s, sigma_s).tofile(p("s"))
            run(0 if top == 255 else 1, B, h, w, s, skew, pad, p("i"), p("g"), p("t"), p("s"), p("o"))
            want = J.want(shape, pattern, top, s, kind, 10.0, sigma_s)
            got = np.fromfile(p("o"), dtype=codes.dtype).reshape(want.shape)
            assert got.tobytes() == want.tobytes(), (shape, name, pattern, layout, kind, sigma_s)
            cases += 1
    return cases, (f"over {len(F.SHAPES)} shapes x {len(J.FORMATS)} formats x {len(F.PATTERNS)} patterns, the guides, sigmas and "
                   "layouts of the guidance in turn: no report, every output equals tests/jbu_ref.py")


def register(run, p):
    """The GPU test's cases (register_ref.cases): every shape under every pattern and calibration, the formats in turn."""
    cases = 0
    for shape in G.SHAPES:
        B, hs, ws, ho, wo = shape[:5]
        for name, top, pattern, calib in G.cases(shape):
            A, T, P = G.tables(shape, calib, top)
            codes = G.plane(shape, pattern, top)
            codes.tofile(p("i")), A.tofile(p("a"))
            np.concatenate([T, P.astype(np.int64)]).tofile(p("p"))
            run(0 if top == 255 else 1, B, hs, ws, top, ho, wo, p("i"), p("a"), p("p"), p("o"), p("s"))
            want, stats = G.want(shape, pattern, top, calib)
            got = np.fromfile(p("o"), dtype=codes.dtype).reshape(want.shape)
            assert got.tobytes() == want.tobytes(), (shape, name, pattern, calib)
            assert np.fromfile(p("s"), dtype=np.uint32).tobytes() == stats.tobytes(), (shape, name, pattern, calib, "statistics")
            cases += 1
    return cases, (f"over {len(G.SHAPES)} shapes x {len(G.PATTERNS)} patterns x {len(G.CALIBS)} calibrations, the {len(G.FORMATS)} formats "
                   "in turn: no report, every output equals tests/register_ref.py")


def clean(run, p):
    """The GPU test's cases (clean_ref.cases): every shape under every pattern and parameter form, the formats in turn; the program
    runs each in both thread orders, with and without statistics"""
    cases = 0
    for shape in K.SHAPES:
        B, h, w = shape
        for name, top, pattern, form in K.cases(shape):
            codes = K.plane(shape, pattern, top)
            codes.tofile(p("i"))
            run(0 if top == 255 else 1, B, h, w, *K.params(shape, form, top, pattern), p("i"), p("o"), p("s"))
            want, stats = K.want(shape, pattern, top, form)
            got = np.fromfile(p("o"), dtype=codes.dtype).reshape(want.shape)
            assert got.tobytes() == want.tobytes(), (shape, name, pattern, form)
            assert np.fromfile(p("s"), dtype=np.uint32).tobytes() == stats.tobytes(), (shape, name, pattern, form, "statistics")
            cases += 1
    return cases, (f"over {len(K.SHAPES)} shapes x {len(K.PATTERNS)} patterns x {len(K.FORMS)} parameter forms, the {len(K.FORMATS)} "
                   "formats in turn: no report, every output and count equals tests/clean_ref.py")


def undistort(run, p):
    """The GPU test's cases (undistort_ref.cases): every shape under every rig and pattern, the images on a 16-byte boundary and
    one byte off it in turn; the tile table and the counts the program made with ud_tiles beside the output"""
    U.weight_table().tofile(p("k"))
    cases = 0
    for shape in U.SHAPES:
        B, H, W, C, ho, wo = shape
        for rig, pattern in U.cases(shape):
            M, tiles, counts = U.tables(shape, rig)
            M.tofile(p("m")), U.image(shape, pattern).tofile(p("i"))
            run(C, B, H, W, ho, wo, cases % 2, p("i"), p("m"), p("k"), p("o"), p("t"), p("c"))
            assert np.fromfile(p("o"), dtype=np.uint8).tobytes() == U.want(shape, rig, pattern).tobytes(), (shape, rig, pattern)
            assert np.fromfile(p("t"), dtype=np.int32).tobytes() == tiles.tobytes(), (shape, rig, "tile table")
            assert np.fromfile(p("c"), dtype=np.uint32).tobytes() == counts.tobytes(), (shape, rig, "counts")
            cases += 1
    return cases, (f"over {len(U.SHAPES)} shapes x {len(U.RIGS)} rigs x {len(U.PATTERNS)} patterns: no report, every output, tile "
                   "table and count equals tests/undistort_ref.py")


def cloud(run, p):
    """The GPU test's cases (cloud_ref.cases): every shape under every pattern and record form; the program runs each in both
    thread orders, with the body and the normal map one byte into their buffers"""
    cases = 0
    for shape in Q.SHAPES:
        B, h, w = shape
        rx, ry = Q.tables(shape)
        rx.tofile(p("x")), ry.tofile(p("y"))
        for pattern, form in Q.cases(shape):
            top = Q.top_of(pattern)
            normals, channels, radius, A, Rq, nmap = Q.params(form, top)
            codes = Q.plane(shape, pattern)
            codes.tofile(p("i"))
            if channels:
                Q.tint(shape, channels).tofile(p("c"))
            run(0 if top == 255 else 1, B, h, w, int(normals), channels, radius, A, Rq, repr(Q.DEFAULTS["depth_unit"] / (1 << 20)),
                int(nmap), p("i"), p("x"), p("y"), p("c"), p("b"), p("n"), p("m"))
            bodies, counts, maps, rec = Q.want(shape, pattern, form)
            got = np.fromfile(p("b"), dtype=np.uint8).reshape(B, h * w * rec)
            for b, body in enumerate(bodies):
                assert got[b, :len(body)].tobytes() == body, (shape, pattern, form, b)
                assert (got[b, len(body):] == 0xEE).all(), (shape, pattern, form, b, "bytes behind the records")
            assert np.fromfile(p("n"), dtype=np.uint32).tobytes() == counts.tobytes(), (shape, pattern, form, "counts")
            if nmap:
                assert np.fromfile(p("m"), dtype=np.uint8).tobytes() == maps.tobytes(), (shape, pattern, form, "normal map")
            cases += 1
    return cases, (f"over {len(Q.SHAPES)} shapes, {len(Q.PATTERNS)} patterns x {len(Q.FORMS)} record forms ({len(Q.BIG_CASES)} of them on "
                   "the largest): no report, every byte and count equals tests/cloud_ref.py")


def mesh(run, p):
    """The GPU test's cases (mesh_ref.cases): every shape under every pattern and tolerance; the program runs each in both thread
    orders, with the face buffer one byte into its allocation"""
    cases = 0
    for shape in H.SHAPES:
        B, h, w = shape
        for pattern, tol in H.cases(shape):
            top = H.top_of(pattern)
            codes = H.plane(shape, pattern)
            codes.tofile(p("i"))
            run(0 if top == 255 else 1, B, h, w, H.tolerance_of(tol, top), H.RQ, p("i"), p("f"), p("n"))
            bodies, counts = H.want(shape, pattern, tol)
            got = np.fromfile(p("f"), dtype=np.uint8).reshape(B, H.row_bytes(h, w))
            for b, body in enumerate(bodies):
                assert got[b, :len(body)].tobytes() == body, (shape, pattern, tol, b)
                assert (got[b, len(body):] == 0xEE).all(), (shape, pattern, tol, b, "bytes behind the faces")
            assert np.fromfile(p("n"), dtype=np.uint32).tobytes() == counts.tobytes(), (shape, pattern, tol, "counts")
            cases += 1
    return cases, (f"over {len(H.SHAPES)} shapes, {len(H.PATTERNS)} patterns x {len(H.TOLERANCES)} tolerances ({len(H.BIG_CASES)} of them "
                   "on the largest): no report, every byte and count equals tests/mesh_ref.py")


def normal_errors(run, p):
    """The GPU test's cases (normal_errors_ref.cases): every shape under every pattern, radius and noise; the program runs each in
    both thread orders.  Then the per-pair index function over pairs no scene reaches: opposite normals, pairs on a threshold,
    D < 0"""
    ctab, stab = (t.astype(np.int32) for t in N.angle_tables())
    ctab.tofile(p("c")), stab.tofile(p("s"))
    cases = 0
    for shape in N.SHAPES:
        B, h, w = shape
        _, hl, wl = N.label_shape(shape)
        rx, ry = N.tables(shape)
        rx.tofile(p("x")), ry.tofile(p("y"))
        for pattern, radius, noise, holes in N.cases(shape):
            top = Q.top_of(pattern)
            label, out = N.planes(shape, pattern, noise, holes)
            label.tofile(p("l")), out.tofile(p("o"))
            run("planes", 0 if top == 255 else 1, B, h, w, hl, wl, radius, N.tolerance_of(top), N.RQ, p("l"), p("o"), p("x"), p("y"),
                p("c"), p("s"), p("r"))
            words, maps = N.want(shape, pattern, radius, noise, holes)
            what = (shape, pattern, radius, noise, holes)
            assert np.fromfile(p("r.words"), dtype=np.uint32).tobytes() == words.tobytes(), (*what, "words")
            assert np.fromfile(p("r.map"), dtype=np.uint16).tobytes() == maps.tobytes(), (*what, "angle map")
            cases += 1
    rows, kinds = N.pairs()
    rows.tofile(p("q"))
    run("pairs", len(rows), p("q"), p("c"), p("s"), p("a"))
    got = np.fromfile(p("a"), dtype=np.int32)
    assert np.array_equal(got, N.index_count(rows[:, :3], rows[:, 3:])), "the index of a pair"
    assert (got[kinds["opposite"]] == N.ANGLES).all() and (got[kinds["same"]] == 0).all()
    assert (N.dot_and_root(rows[:, :3], rows[:, 3:])[0][kinds["random"]] < 0).sum() > 1000
    return cases, (f"over {len(N.SHAPES)} shapes, {len(N.PATTERNS)} patterns x {len(N.RADII)} radii x the noises, and {len(rows)} pairs of "
                   "normals: no report, every word and map equals tests/normal_errors_ref.py")


def temporal(run, p):
    """The GPU test's cases (temporal_ref.cases): the planes under the windows at every length, parameters, patterns and formats
    in turn; the program runs each one element into larger buffers and on a 16-byte boundary, in both thread orders, with and
    without statistics"""
    rows = V.cases()
    for case in rows:
        T_, h, w, Bk, Ah, M_, F_, A, Rq, pattern, top = case
        V.sequence(T_, h, w, pattern, top).tofile(p("i"))
        run(0 if top == 255 else 1, T_, h, w, Bk, Ah, A, Rq, M_, F_, V.chunk_frames(T_, h, w, Bk, Ah), p("i"), p("o"), p("s"))
        want, stats = V.want(case)
        assert np.fromfile(p("o"), dtype=want.dtype).tobytes() == want.tobytes(), case
        assert np.fromfile(p("s"), dtype=np.uint32).tobytes() == stats.tobytes(), (case, "statistics")
    return len(rows), (f"over {len(V.PLANES)} planes x {len(V.WINDOWS)} windows at every length, the {len(V.PARAMS)} parameter forms, "
                       f"{len(V.PATTERNS)} patterns and {len(V.FORMATS)} formats in turn: no report, every byte and count equals "
                       "tests/temporal_ref.py")


def temporal_push(run, p):
    """The GPU test's cases (temporal_stream_cases.cases): the planes under the windows at every length; the program pushes each
    sequence frame by frame and flushes it, one element into larger buffers and on a 16-byte boundary, in both thread orders, with
    and without statistics; the expectation is the restatement of the whole sequence"""
    rows = W.cases()
    for case in rows:
        T_, h, w, Bk, Ah, M_, F_, A, Rq, pattern, top = case
        V.sequence(T_, h, w, pattern, top).tofile(p("i"))
        run(0 if top == 255 else 1, T_, h, w, Bk, Ah, A, Rq, M_, F_, p("i"), p("o"), p("s"))
        want, stats = V.want(case)
        assert np.fromfile(p("o"), dtype=want.dtype).tobytes() == want.tobytes(), case
        assert np.fromfile(p("s"), dtype=np.uint32).tobytes() == stats.tobytes(), (case, "statistics")
    return len(rows), (f"over {len(V.PLANES)} planes x {len(V.WINDOWS)} windows at every length, pushed frame by frame and flushed: "
                       "no report, every byte and count equals tests/temporal_ref.py")


def smooth(run, p):
    """The GPU test's cases (smooth_ref.cases): every plane under every (radius, passes) with the pair rule on and off, the rest in
    turn; the program runs each with the passes split over the launches in every way, one element into larger buffers and on a
    16-byte boundary, in both thread orders, with and without statistics"""
    rows = Y.cases()
    for case in rows:
        B, h, w, R, P, sigma, pairs, A, Rq, pattern, top = case
        Y.codes_of(case).tofile(p("i")), Y.weight_table(R, sigma).tofile(p("w"))
        run(0 if top == 255 else 1, B, h, w, R, P, int(pairs), A, Rq, p("i"), p("w"), p("o"), p("s"))
        want, stats = Y.want(case)
        assert np.fromfile(p("o"), dtype=want.dtype).tobytes() == want.tobytes(), case
        assert np.fromfile(p("s"), dtype=np.uint32).tobytes() == stats.tobytes(), (case, "statistics")
    return len(rows), (f"over {len(Y.PLANES)} planes x {len(Y.RADII)} radii x {len(Y.PASSES)} pass counts x the pair rule on and off, "
                       f"{len(Y.SIGMAS)} sigmas, {len(Y.TOLERANCES)} tolerances, {len(Y.FORMATS)} formats and {len(Y.PATTERNS)} patterns in "
                       "turn: no report, every byte and count equals tests/smooth_ref.py")


# name -> (check, extra compile flags, what the count counts)
CHECKS = {
    "d4": (d4, ["-ffp-contract=off"], "runs"),
    "sensor": (sensor, ["-ffp-contract=off"], "cases"),
    "eval": (eval_, [], "cases"),
    "fill": (fill, [], "cases"),
    "stretch": (stretch, [], "cases"),
    "guided_fill": (guided_fill, [], "cases"),
    "jbu": (jbu, [], "cases"),
    "register": (register, [], "cases"),
    "clean": (clean, [], "cases"),
    "undistort": (undistort, [], "cases"),
    "cloud": (cloud, [], "cases"),
    "mesh": (mesh, [], "cases"),
    "normal_errors": (normal_errors, [], "cases"),
    "temporal": (temporal, [], "cases"),
    "temporal_push": (temporal_push, [], "cases"),
    "smooth": (smooth, [], "cases"),
}


def check(name, cxx):
    fn, extra, noun = CHECKS[name]
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, f"{name}_host_check")
        subprocess.run([cxx, *FLAGS, *extra, os.path.join(ROOT, "tools", f"{name}_host_check.cpp"), "-o", exe], check=True)
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
        count, tail = fn(lambda *args: subprocess.run([exe, *map(str, args)], check=True, env=env, stdout=subprocess.DEVNULL),
                         lambda n: os.path.join(tmp, n))
    print(f"{name}_host_check: {count} {noun} under -fsanitize=address,undefined {tail}", flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("name", choices=[*CHECKS, "all"])
    ap.add_argument("--cxx", default=default_cxx(), help="a clang++ with the sanitizer runtimes")
    a = ap.parse_args(argv)
    for name in (CHECKS if a.name == "all" else [a.name]):
        check(name, a.cxx)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
