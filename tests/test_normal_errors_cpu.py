"""The surface-normal angle error without a GPU: the premises of the integer angle index -- the tables, the single
crossing that lets the kernel bisect, the ends of the scale, the distance to a float64 atan2 -- the numpy restatement
tests/normal_errors_ref.py on inputs where the metric is not idle, metrics.normal_report on hand-made rows, and every refusal of
the C entry (on the host, before any HIP call), of metrics.normal_errors' host checks and of the command line."""
import ctypes as C
import math
import re

import numpy as np
import pytest

from codon_amd import _lib as L
from codon_amd import infer, metrics
from tests import normal_errors_ref as N


# ---- the premises ---------------------------------------------------------------------------------------------------------------------

def test_tables():
    c, s = metrics.angle_tables()
    wc, ws = N.angle_tables()
    assert c.dtype == s.dtype == np.int32 and c.shape == s.shape == (N.ANGLES,)
    assert np.array_equal(c, wc) and np.array_equal(s, ws)
    assert (np.diff(wc) < 0).all()                                    # the cosine falls strictly over 0 .. 180 degrees
    half = N.ANGLES // 2
    assert (np.diff(ws[:half]) > 0).all() and (np.diff(ws[half:]) < 0).all() and ws[half - 1] == ws[half]
    assert ws.min() == N.S_MIN == ws[0] == ws[-1] and np.abs(wc).max() <= 1 << 30 and ws.max() <= 1 << 30
    assert np.array_equal(wc, -wc[::-1]) and np.array_equal(ws, ws[::-1])
    # every product of the predicate stays below 2^61: A < 2^30 (isqrt of a sum below 2^60), |D| < 2^30
    assert (1 << 30) * int(np.abs(wc).max()) < 1 << 61 and (3 << 28) * int(ws.max()) < 1 << 61


def test_count_equals_bisection_and_the_ends():
    rows, kinds = N.pairs()
    assert kinds["random"].stop >= 20000 and kinds["threshold"].stop - kinds["threshold"].start == 4 * N.ANGLES
    p, q = rows[:, :3], rows[:, 3:]
    count, bisect = N.index_count(p, q), N.index_bisect(p, q)
    assert np.array_equal(count, bisect)
    assert (count[kinds["same"]] == 0).all() and (count[kinds["opposite"]] == N.ANGLES).all()
    # the pairs placed on threshold m land in bin m - 1 or m, and both sides of a threshold are reached
    m = np.repeat(np.arange(1, N.ANGLES + 1), 4)
    on = count[kinds["threshold"]]
    assert ((on == m) | (on == m - 1)).all() and (on == m).sum() > 1000 and (on == m - 1).sum() > 1000
    D, A = N.dot_and_root(p, q)
    assert (D[kinds["random"]] < 0).sum() > 5000 and np.abs(D).max() < 1 << 29 and A.max() < 1 << 29


def test_single_crossing():
    """The predicate holds for every m up to the count and for none beyond: what the bisection rests on"""
    rows, _ = N.pairs()
    C_, S_ = N.angle_tables()
    D, A = N.dot_and_root(rows[:4000, :3], rows[:4000, 3:])
    pred = A[:, None] * C_[None] - D[:, None] * S_[None] > 0
    assert (np.diff(pred.astype(np.int8), axis=1) <= 0).all()


def test_against_float64_atan2():
    rows, _ = N.pairs()
    p, q = rows[:, :3].astype(np.float64), rows[:, 3:].astype(np.float64)
    angle = np.degrees(np.arctan2(np.linalg.norm(np.cross(p, q), axis=1), (p * q).sum(axis=1)))
    a = N.index_count(rows[:, :3], rows[:, 3:])
    worst = np.abs(a / 8.0 - angle).max()
    print(f"|a / 8 - atan2| at most {worst!r} degrees over {len(rows)} pairs")
    assert worst <= 1.0 / 16.0 + 1e-5


# ---- the restatement ------------------------------------------------------------------------------------------------------------------

def test_a_plane_against_itself_is_bin_0():
    shape = N.WINDOWED
    for pattern in ("random", "u8", "high", "surfaces"):
        words, maps = N.want(shape, pattern, 2, "0")
        r = N.report(words[0])
        assert words[0, 0] == words[0, N.COMPARED] > 0 and words[0, 1:N.BINS].sum() == 0 and r["normal_coverage"] > 0
        assert r["normal_mean"] == r["normal_rmse"] == r["normal_median"] == 0.0 and r["normal<11.25"] == 1.0
        assert set(np.unique(maps)) <= {0, N.NONE}


def test_the_metric_is_not_idle():
    """want() asserts the spread on every wide case; here the figures the issue names, on the largest shape"""
    words, _ = N.want(N.WINDOWED, "random", 2, "wide")
    bins = np.flatnonzero(words[0, :N.BINS])
    assert bins.size >= 64 and bins.max() > 720
    few, _ = N.want(N.WINDOWED, "random", 2, "1")
    assert 2 <= np.flatnonzero(few[0, :N.BINS]).size < bins.size
    holes, _ = N.want(N.WINDOWED, "random", 2, "1", True)
    assert holes[0, N.OUT_HOLES] > 100 and holes[0, N.COMPARED] < few[0, N.COMPARED]


def test_the_mask_hides_what_the_output_holds_in_the_labels_holes():
    shape = (1, 32, 32)
    label, out = N.planes(shape, "random", "1")
    rx, ry = N.tables(shape)
    other = np.where(label[:, :32, :32] == 0, 7, out)
    a = N.normal_errors(label, out, rx, ry, 2, 20, N.RQ)
    b = N.normal_errors(label, other.astype(out.dtype), rx, ry, 2, 20, N.RQ)
    assert (out[label == 0] != 0).all() and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_every_case_runs_and_the_counts_are_what_the_test_files_pin():
    n = sum(len(N.cases(s)) for s in N.SHAPES)
    assert n == 336 and len(N.SHAPES) == 7


# ---- the report -----------------------------------------------------------------------------------------------------------------------

def _row(hist: dict, valid, label_normals=None, out_holes=0):
    w = np.zeros(N.WORDS, dtype=np.int64)
    for a, v in hist.items():
        w[a] = v
    n = sum(hist.values())
    w[N.VALID], w[N.LABEL_NORMALS], w[N.COMPARED], w[N.OUT_HOLES] = valid, n if label_normals is None else label_normals, n, out_holes
    return w


def test_report_on_a_hand_made_row():
    # 4 pixels at 0 degrees, 3 at 10 (a = 80), 2 at 22.5 (a = 180), 1 at 90 (a = 720): n = 10 of 16 valid
    r = metrics.normal_report(_row({0: 4, 80: 3, 180: 2, 720: 1}, 16))
    assert list(r) == ["normal_n", "normal_coverage", "normal_mean", "normal_rmse", "normal_median", "normal<11.25", "normal<22.5",
                       "normal<30"]
    assert r["normal_n"] == 10 and r["normal_coverage"] == 10 / 16
    assert r["normal_mean"] == (3 * 10 + 2 * 22.5 + 90) / 10 == 16.5
    assert r["normal_rmse"] == math.sqrt((3 * 80 * 80 + 2 * 180 * 180 + 720 * 720) / 10) / 8
    assert r["normal_median"] == 10.0                                 # the fifth pixel of ten: ceil(10 / 2) = 5 is reached at a = 80
    assert r["normal<11.25"] == 0.7 and r["normal<22.5"] == 0.9 and r["normal<30"] == 0.9
    assert r == N.report(_row({0: 4, 80: 3, 180: 2, 720: 1}, 16))
    odd = metrics.normal_report(_row({8: 1, 16: 1, 1440: 1}, 3), thresholds=(1.0, 2.0, 180, 0))
    assert odd["normal_median"] == 2.0 and odd["normal<1"] == 1 / 3 and odd["normal<2"] == 2 / 3 and odd["normal<180"] == 1.0
    assert odd["normal<0"] == 0.0 and odd["normal_mean"] == (1 + 2 + 180) / 3
    # int32 words as the device tensor holds them, and a threshold exactly on a bin counts the bin
    assert metrics.normal_report(_row({90: 2}, 2).astype(np.int32), thresholds=(11.25,))["normal<11.25"] == 1.0
    assert metrics.normal_report(_row({91: 2}, 2).astype(np.int32), thresholds=(11.25,))["normal<11.25"] == 0.0


def test_report_without_compared_pixels_is_nan_and_the_means_skip_it():
    r = metrics.normal_report(_row({}, 12, label_normals=0))
    assert r["normal_n"] == 0 and r["normal_coverage"] == 0.0
    assert all(math.isnan(r[k]) for k in ("normal_mean", "normal_rmse", "normal_median", "normal<11.25", "normal<22.5", "normal<30"))
    assert math.isnan(metrics.normal_report(_row({}, 0))["normal_coverage"])
    full = metrics.normal_report(_row({16: 4}, 4))
    means = metrics.report_means([r, full])
    assert means["normal_mean"] == [2.0, 1] and means["normal_coverage"] == [0.5, 2] and "normal_n" not in means


@pytest.mark.parametrize("thresholds, word", [
    ((11.3,), "threshold 11.3 "), ((-0.125,), "threshold -0.125 "), ((180.125,), "threshold 180.125 "), ((float("nan"),), "threshold nan "),
    (("30",), "threshold '30' "), ((True,), "threshold True "), ((1, 2, 3, 4, 5), "5 thresholds \\(at most 4\\)")])
def test_report_refuses_a_bad_threshold(thresholds, word):
    with pytest.raises(ValueError, match="normal_report: " + word):
        metrics.normal_report(_row({0: 1}, 1), thresholds=thresholds)


def test_report_refuses_a_row_of_another_length_or_a_broken_one():
    with pytest.raises(ValueError, match="normal_report: 16 words"):
        metrics.normal_report(np.zeros(16, dtype=np.int64))
    bad = _row({0: 3}, 3)
    bad[N.COMPARED] = 2
    with pytest.raises(ValueError, match="the histogram holds 3 pixels"):
        metrics.normal_report(bad)


# ---- the C entry ----------------------------------------------------------------------------------------------------------------------

def normal_caller(lib, label, out, rx, ry, ctab, stab, words, amap=None, stream=None):
    """The good call of normal_errors_ref.REFUSALS -- u16 codes, a 5 x 7 window of a 6 x 9 label -- over the given addresses, with
    what a refusal changes as keyword arguments; shared with the GPU test"""
    P_ = C.c_void_p

    def call(B=1, h=5, w=7, label=label, hl=6, wl=9, row=9, image=54, out=out, fmt=L.FILL_U16, top=65535, rx=rx, ry=ry,
             span=(-100, 100, -90, 90), ctab=ctab, stab=stab, radius=2, tol_abs=2, tol_rel=N.RQ, words=words, amap=amap):
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_normal_errors(B, h, w, p(label), hl, wl, row, image, p(out), fmt, top, p(rx), p(ry),
                                     None if span is None else (C.c_int32 * 4)(*span), p(ctab), p(stab), radius, tol_abs, tol_rel,
                                     p(words), p(amap), stream)
        return st, lib.codon_last_error_string().decode()
    return call


def normal_refusals(lib, call):
    for kw, word in N.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("normal_errors: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="normal_errors failed with status -1: normal_errors: "):
            L.check(st, "normal_errors")


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    call = normal_caller(lib, 4096, 8192, 12288, 16384, 20480, 24576, 28672)    # never dereferenced: every call is refused on the host
    normal_refusals(lib, call)
    for kw in ({"label": 4097}, {"out": 8193}, {"rx": 12290}, {"ry": 16385}, {"ctab": 20482}, {"stab": 24577}, {"words": 28674},
               {"amap": 32769}):
        assert "unaligned" in call(**kw)[1], kw
    # u8 planes need no alignment: at the bounds themselves, with odd planes, the refusal is the next rule's
    at = dict(fmt=L.FILL_U8, top=255, label=4097, out=8193, tol_abs=255, tol_rel=65535, radius=8, span=(-(1 << 22) + 1, (1 << 22) - 1, 0, 0))
    assert "unaligned plane, table, words or map" in call(**at, words=28674)[1]
    assert "radius 9 " in call(**{**at, "radius": 9})[1]


# ---- metrics.normal_errors' host checks and the command line ----------------------------------------------------------------------------

def test_normal_errors_refuses_on_the_host():
    import torch
    from codon_amd import register as P
    lab, out = torch.zeros((6, 9), dtype=torch.uint8), torch.zeros((5, 7), dtype=torch.uint8)
    cam = P.Camera(9, 6, 10.0, 10.0, 4.0, 3.0)
    for kw, word in (
            (dict(camera=P.Camera(9, 6, 10.0, 10.0, 4.0, 3.0, (0.1, 0, 0, 0, 0))), "camera.dist .* is not zero"),
            (dict(camera=P.Camera(6, 6, 10.0, 10.0, 4.0, 3.0)), "a 6x6 camera is smaller than the 5x7 output"),
            (dict(camera=P.Camera(9, 4, 10.0, 10.0, 4.0, 3.0)), "a 4x9 camera is smaller than the 5x7 output"),
            (dict(camera="cam"), "camera must be a register.Camera or a pair"),
            (dict(camera=(np.zeros(6, dtype=np.int32), np.zeros(6, dtype=np.int32))), "ray tables of a 6x6 camera are smaller"),
            (dict(camera=(np.zeros(9, dtype=np.int64), np.zeros(6, dtype=np.int32))), "camera must be .* a pair of int32 ray tables"),
            (dict(camera=(np.full(9, 1 << 22, dtype=np.int32), np.zeros(6, dtype=np.int32))), "a ray of 2\\^22 or more"),
            (dict(radius=0), "radius 0 "), (dict(radius=9), "radius 9 "), (dict(tolerance=-1), "tolerance -1 "),
            (dict(tolerance=256), "tolerance 256 "), (dict(tolerance_rel=1.0), "tolerance_rel 1.0 "),
            (dict(depth_max=1000), "depth_max 1000 with 8-bit codes")):
        with pytest.raises(ValueError, match="normal_errors: " + word):
            metrics.normal_errors(lab, out, **{"camera": cam, **kw})
    with pytest.raises(ValueError, match="normal_errors: a 5x7 label is smaller than the 6x9 output"):
        metrics.normal_errors(out, lab, cam)
    with pytest.raises(ValueError, match="normal_errors: label torch.uint8 and output torch.int16"):
        metrics.normal_errors(lab, out.to(torch.int16), cam)


BASE = ["--lr-depth", "d", "--input-color", "c", "--label", "l"]
NORMALS = [*BASE, "--report", "--report-normals", "--calib", "rig.json"]


@pytest.mark.parametrize("argv, word", [
    ([*BASE, "--report", "--report-normals"], "--report-normals needs --calib"),
    ([*BASE, "--report", "--calib", "rig.json"], "--calib needs --report-normals"),
    ([*BASE, "--report-normals", "--calib", "rig.json"], "--report-normals needs --report"),
    ([*BASE, "--report", "--camera", "depth"], "--camera needs --report-normals"),
    ([*BASE, "--report", "--normal-radius", "3"], "--normal-radius needs --report-normals"),
    ([*BASE, "--report", "--normal-tolerance", "3"], "--normal-tolerance needs --report-normals"),
    ([*BASE, "--report", "--normal-tolerance-rel", "0.1"], "--normal-tolerance-rel needs --report-normals"),
    ([*BASE, "--report", "--normal-thresholds", "5"], "--normal-thresholds needs --report-normals"),
    ([*BASE, "--report", "--normal-error-maps", "m"], "--normal-error-maps needs --report-normals"),
    ([*NORMALS, "--camera", "ir"], "invalid choice"),
    ([*NORMALS, "--normal-radius", "0"], "--normal-radius 0 must be in \\[1, 8\\]"),
    ([*NORMALS, "--normal-radius", "9"], "--normal-radius 9 must be in \\[1, 8\\]"),
    ([*NORMALS, "--normal-tolerance", "-1"], "--normal-tolerance -1 must be in \\[0, 255\\]"),
    ([*NORMALS, "--normal-tolerance", "256"], "--normal-tolerance 256 must be in \\[0, 255\\]"),
    ([*NORMALS, "--depth-bits", "16", "--depth-max", "10000", "--normal-tolerance", "10001"],
     "--normal-tolerance 10001 must be in \\[0, 10000\\]"),
    ([*NORMALS, "--normal-tolerance-rel", "1.0"], "--normal-tolerance-rel 1.0 must be in \\[0, 1\\)"),
    ([*NORMALS, "--normal-thresholds", "11.3"], "--normal-thresholds .*threshold 11.3 "),
    ([*NORMALS, "--normal-thresholds", "1,2,3,4,5"], "--normal-thresholds .*5 thresholds"),
    ([*NORMALS, "--normal-thresholds", "a,b"], "--normal-thresholds 'a,b': degrees, separated by commas"),
    ([*NORMALS, "--normal-error-maps", "l/"], "--normal-error-maps is a directory of inputs"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        infer.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_command_line_defaults():
    a, _ = infer.parse_args(NORMALS)
    assert a.report_normals and a.calib == "rig.json"
    assert a.normals == {"calib": "rig.json", "camera": "color", "radius": 2, "tolerance": 2, "tolerance_rel": 0.02,
                         "thresholds": (11.25, 22.5, 30.0), "error_maps": None}
    b, _ = infer.parse_args([*NORMALS, "--camera", "depth", "--normal-radius", "8", "--normal-thresholds", "5,180", "--normal-error-maps", "m"])
    assert b.normals["camera"] == "depth" and b.normals["radius"] == 8 and b.normals["thresholds"] == (5.0, 180.0) and b.normals["error_maps"] == "m"
    c, _ = infer.parse_args([*BASE, "--report"])
    assert c.normals is None
