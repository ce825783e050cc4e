"""The surface-normal angle error on the MI355X against the numpy restatement tests/normal_errors_ref.py (pinned on
the CPU by tests/test_normal_errors_cpu.py).  The bar is EQUAL WORDS and EQUAL MAPS, no tolerance anywhere.
Shapes (normal_errors_ref.SHAPES), the smallest at which each part can go wrong: one pixel; a single row; 5 x 7, where nothing is
compared at radius 8; exactly one tile; a second tile of one pixel each way, so the halo crosses tile borders; a batch of three,
for the per-image rows; 93 x 116, many tiles, the label a window of a larger plane read by its strides.
Every shape under every pattern, radius (1, 2, 8) and noise (normal_errors_ref.cases): u8, u16 and codes of 32768 and above, an
occlusion edge, a checkerboard of holes, no valid pixel at all, an output with holes inside valid label.  In every case every
buffer starts one element into a larger one, the words and the map are prefilled with garbage, and nothing outside them is
written."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, metrics, ops
from codon_amd import register as P
from tests import cloud_ref as Q
from tests import normal_errors_ref as N
from tests.test_normal_errors_cpu import normal_caller, normal_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731
FILL = 0x5A5A
C_INT4 = C.c_int32 * 4


def _stream():
    return ops._stream(torch.device("cuda:0"))


def _offset(a, fill=0):
    """numpy array -> (the device buffer that holds it one element in, a view of it there)"""
    a = np.ascontiguousarray(a)
    a = a.view(np.int16) if a.dtype == np.uint16 else a
    buf = torch.full((a.size + 2,), fill, dtype=torch.from_numpy(a[:0].copy()).dtype, device="cuda")
    buf[1:a.size + 1] = torch.from_numpy(a.reshape(-1).copy()).cuda()
    return buf, buf[1:a.size + 1].view(a.shape)


@pytest.fixture(scope="module")
def angle_tabs():
    c, s = metrics.angle_tables()
    return _offset(c, 7), _offset(s, 7)


class Raw:
    """One case through the C entry, every buffer one element into a larger one"""

    def __init__(self, shape, tabs, pattern, radius, noise, holes=False):
        self.shape, self.key = shape, (pattern, radius, noise, holes)
        B, h, w = shape
        self.top, self.radius = Q.top_of(pattern), radius
        label, out = N.planes(shape, pattern, noise, holes)
        if pattern == "high":
            assert (label.view(np.int16) < 0).sum() > 0               # as an int16 view, negative
        self.label_buf, self.label = _offset(label, 1)
        self.out_buf, self.out = _offset(out, 1)
        rx, ry = N.tables(shape)
        self.span = C_INT4(int(rx[0]), int(rx[w - 1]), int(ry[0]), int(ry[h - 1]))
        (self.rx_buf, self.rx), (self.ry_buf, self.ry) = _offset(rx, 1 << 21), _offset(ry, 1 << 21)
        (_, self.ctab), (_, self.stab) = tabs
        self.words = torch.full((B * N.WORDS + 2,), 0x7A7A7A7A, dtype=torch.int32, device="cuda")
        self.map = torch.full((B * h * w + 2,), FILL, dtype=torch.int16, device="cuda")

    def run(self, stream=None, with_map=True):
        B, h, w = self.shape
        _, hl, wl = self.label.shape
        P_ = C.c_void_p
        st = L.load().codon_normal_errors(B, h, w, P_(self.label.data_ptr()), hl, wl, wl, hl * wl, P_(self.out.data_ptr()),
                                          L.FILL_U8 if self.top == 255 else L.FILL_U16, self.top, P_(self.rx.data_ptr()),
                                          P_(self.ry.data_ptr()), self.span, P_(self.ctab.data_ptr()), P_(self.stab.data_ptr()),
                                          self.radius, N.tolerance_of(self.top), N.RQ, P_(self.words.data_ptr() + 4),
                                          P_(self.map.data_ptr() + 2) if with_map else None, _stream() if stream is None else stream)
        L.check(st, "normal_errors")

    def check(self, with_map=True):
        B, h, w = self.shape
        words, maps = N.want(self.shape, *self.key)
        what = (self.shape, *self.key)
        torch.cuda.synchronize()
        got = self.words.cpu().numpy()
        assert got[0] == 0x7A7A7A7A and got[-1] == 0x7A7A7A7A, (what, "a word outside the rows was written")
        got = got[1:-1].view(np.uint32).reshape(B, N.WORDS)
        bad = np.argwhere(got != words)
        assert bad.size == 0, f"{what}: {len(bad)} words differ, the first (image, word) {bad[0].tolist()}: {got[tuple(bad[0])]} for {words[tuple(bad[0])]}"
        m = self.map.cpu().numpy().view(np.uint16)
        assert m[0] == FILL and m[-1] == FILL, (what, "a texel outside the map was written")
        if with_map:
            assert np.array_equal(m[1:-1].reshape(maps.shape), maps), (what, "angle map", int((m[1:-1].reshape(maps.shape) != maps).sum()))
        else:
            assert (m == FILL).all(), (what, "the map was written without being asked for")
        for buf, edge in ((self.label_buf, 1), (self.out_buf, 1), (self.rx_buf, 1 << 21), (self.ry_buf, 1 << 21)):
            assert buf[0] == edge and buf[-1] == edge


@pytest.mark.parametrize("shape", N.SHAPES, ids=ids)
def test_equals_the_restatement(shape, angle_tabs):
    """normal_errors_ref.cases: every pattern under every radius and noise, and the output with holes"""
    for key in N.cases(shape):
        case = Raw(shape, angle_tabs, *key)
        case.run()
        case.check()


def test_what_the_case_set_covers():
    """From the restatement: nothing is compared on 5 x 7 at radius 8 and on the checkerboard at radius 1; the wide cases spread
    over many bins and past 90 degrees; word 1444 counts; the larger shapes take more than one tile"""
    assert (N.want(N.SHAPES[2], "random", 8, "wide")[0][:, N.COMPARED] == 0).all()
    assert (N.want(N.WINDOWED, "checker", 1, "wide")[0][:, N.COMPARED] == 0).all()
    wide = N.want(N.WINDOWED, "random", 2, "wide")[0][0]
    assert np.flatnonzero(wide[:N.BINS]).size >= 64 and np.flatnonzero(wide[:N.BINS]).max() > 720
    assert N.want(N.WINDOWED, "random", 2, "1", True)[0][0, N.OUT_HOLES] > 100
    assert (N.want(N.WINDOWED, "none", 2, "0")[0] == 0).all()
    assert N.label_shape(N.WINDOWED) == (1, 98, 123) and -(-33 // 32) == 2


def test_without_a_map_a_second_call_a_side_stream_and_the_python_interface(angle_tabs):
    """The entry zeroes the words itself: a second call on the same buffers with another output equals its own restatement; a call
    without a map writes none.  A call on a side stream.  metrics.normal_errors gives the same words and maps: a batch with the
    label a window read by its strides, int16 and uint16 carriers, a single (H, W) plane, u8, a pair of tables for a camera"""
    shape = N.WINDOWED
    case = Raw(shape, angle_tabs, "random", 2, "wide")
    case.run(with_map=False)
    case.check(with_map=False)
    case.run()
    case.check()
    other = Raw(shape, angle_tabs, "random", 2, "1", True)
    case.out.copy_(other.out)
    case.key = other.key
    case.run()
    case.check()
    side = torch.cuda.Stream()
    third = Raw(shape, angle_tabs, "surfaces", 8, "wide")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        third.run(stream=ops._stream(torch.device("cuda:0")))
    third.check()
    # the Python entry
    B, h, w = shape
    _, hl, wl = N.label_shape(shape)
    cam = P.Camera(wl, hl, *Q.camera_of(shape))
    label, out = N.planes(shape, "random", "wide")
    lab = torch.from_numpy(np.array(label).view(np.int16)).cuda()
    o16 = torch.from_numpy(np.array(out).view(np.int16)).cuda()
    words, maps = N.want(shape, "random", 2, "wide")
    tol = N.tolerance_of(10000)
    got, amap = metrics.normal_errors(lab, o16, cam, tolerance=tol, depth_max=10000, angle_map=True)
    assert got.dtype == torch.int32 and got.shape == (1, N.WORDS) and amap.dtype == torch.uint16 and amap.shape == (1, h, w)
    assert np.array_equal(got.cpu().numpy().view(np.uint32), words) and np.array_equal(amap.cpu().numpy(), maps)
    with torch.cuda.stream(side):
        single = metrics.normal_errors(lab[0].view(torch.uint16), o16[0], N.tables(shape), tolerance=tol, depth_max=10000, angle_map=True)
    side.synchronize()
    assert single[0].shape == (1, N.WORDS) and single[1].shape == (h, w)
    assert np.array_equal(single[0].cpu().numpy().view(np.uint32), words) and np.array_equal(single[1].cpu().numpy(), maps[0])
    alone = metrics.normal_errors(lab, o16.view(torch.uint16), cam, tolerance=tol, depth_max=10000)
    assert isinstance(alone, torch.Tensor) and np.array_equal(alone.cpu().numpy().view(np.uint32), words)
    r = metrics.normal_report(alone[0].cpu())
    assert r == N.report(words[0]) and r["normal_n"] == int(words[0, N.COMPARED]) and 0 < r["normal<11.25"] < r["normal<30"] <= 1
    shape8 = N.SHAPES[5]
    l8, o8 = N.planes(shape8, "u8", "wide")
    got8 = metrics.normal_errors(torch.from_numpy(np.array(l8)).cuda(), torch.from_numpy(np.array(o8)).cuda(),
                                 P.Camera(shape8[2], shape8[1], *Q.camera_of(shape8)), radius=1, tolerance=N.tolerance_of(255))
    assert np.array_equal(got8.cpu().numpy().view(np.uint32), N.want(shape8, "u8", 1, "wide")[0])
    with pytest.raises(ValueError, match="normal_errors: a 98x123 camera is smaller than the"):
        metrics.normal_errors(torch.zeros((1, 99, 123), dtype=torch.uint8, device="cuda"),
                              torch.zeros((1, 99, 123), dtype=torch.uint8, device="cuda"), cam)


def test_refusals_leave_every_output_untouched(angle_tabs):
    lib = L.load()
    shape = N.SHAPES[2]
    case = Raw(shape, angle_tabs, "random", 2, "1")
    label = torch.full((6 * 9 + 2,), 1, dtype=torch.int16, device="cuda")
    call = normal_caller(lib, label.data_ptr() + 2, case.out.data_ptr(), case.rx.data_ptr(), case.ry.data_ptr(), case.ctab.data_ptr(),
                         case.stab.data_ptr(), case.words.data_ptr() + 4, amap=case.map.data_ptr() + 2, stream=_stream())
    normal_refusals(lib, call)
    assert "unaligned" in call(label=label.data_ptr() + 1)[1] and "unaligned" in call(words=case.words.data_ptr() + 2)[1]
    assert "unaligned" in call(amap=case.map.data_ptr() + 1)[1] and "unaligned" in call(rx=case.rx.data_ptr() + 1)[1]
    torch.cuda.synchronize()
    assert (case.words == 0x7A7A7A7A).all() and (case.map == FILL).all()
    case.run()                                                        # and the good call goes through
    case.check()


# ---- the command line ------------------------------------------------------------------------------------------------------------------

def _tokens(r):
    return " ".join(f"{k}={v!r}" for k, v in r.items())


def test_infer_main_reports_the_normals(tmp_path, capsys):
    """--lr-depth --baseline bicubic --label --report --report-normals --calib on a 24 x 40 scene, no weights: pipelined and --serial
    print the same lines; the normal_* tokens, the JSON and the error-map PNGs equal the restatement computed from the written
    output PNGs and the labels (which are larger than the output: read top-left)"""
    top, s, h, w = 10000, 4, 24, 40
    lrd, cd, ld = (str(tmp_path / n) for n in ("lr", "color", "label"))
    for d in (lrd, cd, ld):
        os.makedirs(d)
    cam = dict(width=w + 3, height=h + 2, fx=47.0, fy=45.5, cx=19.25, cy=12.5)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps({"depth": dict(cam, fx=40.0), "color": cam, "rotation": np.eye(3).tolist(), "translation": [0.0, 0.0, 0.0]}))
    g = np.random.default_rng(3)
    i, j = np.meshgrid(np.arange(h + 2), np.arange(w + 3), indexing="ij")
    labels = []
    for k in range(3):
        z = 4000 + 40 * i + (25 + 10 * k) * j + 150 * np.sin(0.3 * i + k) * np.cos(0.2 * j)
        z = np.where(j > 24 + k, z + 1500, z)                          # an occlusion edge
        lab = np.where(g.uniform(size=z.shape) < 0.08, 0, np.rint(z)).astype(np.uint16)
        lr = lab[1:h:s, 2:w:s].copy()
        lr[k, 3] = 0                                                  # a hole in the sensor's map
        io.write_depth16(os.path.join(ld, f"{k:02d}.png"), lab)
        io.write_depth16(os.path.join(lrd, f"{k:02d}.png"), lr)
        io.write_gray(os.path.join(cd, f"{k:02d}.png"), g.integers(0, 256, size=(h, w), dtype=np.uint8))
        labels.append(lab)
    outs = {}
    for mode in ("pipe", "serial"):
        od, md, js = tmp_path / f"out_{mode}", tmp_path / f"maps_{mode}", tmp_path / f"{mode}.json"
        capsys.readouterr()
        rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", ld, "--out", str(od), "--baseline", "bicubic",
                         "--depth-bits", "16", "--depth-max", str(top), "--report", "--report-normals", "--calib", str(rig),
                         "--normal-error-maps", str(md), "--report-json", str(js)] + (["--serial"] if mode == "serial" else []))
        assert rc == 0
        outs[mode] = (capsys.readouterr().out, {n: open(md / n, "rb").read() for n in sorted(os.listdir(md))}, open(js).read())
    assert outs["pipe"] == outs["serial"] and len(outs["pipe"][1]) == 3
    lines = outs["pipe"][0].strip().splitlines()
    doc = json.loads(outs["pipe"][2])
    rx, ry = Q.ray_tables(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    reports = []
    for k, lab in enumerate(labels):
        out = io.read_depth_plane(str(tmp_path / "out_pipe" / f"{k:02d}.png"), 16, top)
        assert out.shape == (h, w)
        words, amap = N.normal_errors_plane(lab, out, rx, ry, 2, 2, N.RQ)
        r = N.report(words)
        assert r["normal_n"] > 200 and r["normal_mean"] > 0, r        # the metric is not idle here
        assert lines[k].startswith(f"{k:02d}.png ") and lines[k].endswith(" " + _tokens(r)) and " mad=" in lines[k]
        image = doc["images"][k]
        assert image["file"] == f"{k:02d}.png" and {key: image[key] for key in r} == r
        png = np.where(amap == N.NONE, 255, np.minimum(254, amap // 8)).astype(np.uint8)
        assert np.array_equal(io.read_gray(str(tmp_path / "maps_pipe" / f"{k:02d}.png")), png), k
        reports.append(r)
    mean = lines[-1]
    assert mean.startswith("mean ")
    for key in ("normal_coverage", "normal_mean", "normal_rmse", "normal_median", "normal<11.25", "normal<22.5", "normal<30"):
        want = sum(r[key] for r in reports) / 3
        assert f" {key}={want!r}/3" in mean + " " and doc["means"][key] == [want, 3]
    assert "normal_n" not in doc["means"] and not any(math.isnan(r["normal_mean"]) for r in reports)
    # a report without the normals prints the lines as before: the depth tokens are a prefix of the lines above
    capsys.readouterr()
    assert infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", ld, "--baseline", "bicubic", "--depth-bits", "16",
                       "--depth-max", str(top), "--report"]) == 0
    plain = capsys.readouterr().out.strip().splitlines()
    assert len(plain) == len(lines) and all(b.startswith(a + " normal_n=") for a, b in zip(plain[:3], lines[:3]))
    assert "normal" not in plain[-1] and lines[-1].startswith(plain[-1] + " normal_coverage=")
