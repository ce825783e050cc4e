"""The point clouds with normals on the MI355X against the numpy restatement tests/cloud_ref.py (pinned on the CPU by
tests/test_cloud_cpu.py).  The bar is EQUAL BYTES, records, counts and normal maps, no tolerance anywhere.
Shapes (cloud_ref.SHAPES), the smallest at which each part can go wrong: one pixel; a single row; odd sizes; exactly one block of
1024 pixels; a second block that holds one pixel; a batch of three, for the per-image offsets; 93 x 116, many blocks whose spans
start at every address modulo 4; 520 x 512, 260 blocks, so a thread of the scan takes more than one block word.
Every shape under every pattern and every record form (cloud_ref.cases; four of them on the largest).  In every case the codes, the
colour, the body and the normal map each start one element, or one byte, into a larger buffer -- the staged 4-byte stores run on
an odd base address -- and the body is prefilled: nothing before its first byte and nothing behind count * rec bytes is written."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import cloud as K
from codon_amd import infer, io, ops
from codon_amd import register as P
from tests import cloud_ref as R
from tests import register_ref as G
from tests.test_cloud_cpu import cloud_caller, cloud_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731
FILL = 0xA7
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


class Raw:
    """One case through the C entry, every buffer one element into a larger one"""

    def __init__(self, shape, pattern, form):
        self.shape, self.pattern, self.form = shape, pattern, form
        B, h, w = shape
        self.top = R.top_of(pattern)
        self.normals, self.channels, self.radius, self.A, self.Rq, self.nmap = R.params(form, self.top)
        self.rec = R.record_dtype(self.normals, self.channels != 0).itemsize
        rx, ry = R.tables(shape)
        self.rx, self.ry = torch.from_numpy(np.array(rx)).cuda(), torch.from_numpy(np.array(ry)).cuda()
        self.span = C_INT4(int(rx[0]), int(rx[-1]), int(ry[0]), int(ry[-1]))
        codes = R.plane(shape, pattern)
        if pattern == "high":
            assert (codes.view(np.int16) < 0).sum() > 0               # as an int16 view, negative
        self.codes_buf, self.codes = _offset(codes, 1)
        self.color_buf, self.color = _offset(R.tint(shape, self.channels), 9) if self.channels else (None, None)
        self.n = B * h * w * self.rec
        self.body = torch.full((self.n + 2,), FILL, dtype=torch.uint8, device="cuda")
        self.map = torch.full((B * h * w * 3 + 2,), FILL, dtype=torch.uint8, device="cuda") if self.nmap else None
        self.counts = torch.full((B, 2), -7, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(L.load().codon_cloud_workspace_bytes(B, h, w), dtype=torch.uint8, device="cuda")

    def run(self, stream=None):
        B, h, w = self.shape
        P_ = C.c_void_p
        st = L.load().codon_cloud_points(B, h, w, P_(self.codes.data_ptr()), L.FILL_U8 if self.top == 255 else L.FILL_U16, self.top,
                                         P_(self.rx.data_ptr()), P_(self.ry.data_ptr()), self.span, R.DEFAULTS["depth_unit"] / (1 << 20),
                                         int(self.normals), self.radius, self.A, self.Rq,
                                         P_(self.color.data_ptr()) if self.channels else None, self.channels,
                                         P_(self.body.data_ptr() + 1), P_(self.counts.data_ptr()),
                                         P_(self.map.data_ptr() + 1) if self.nmap else None, P_(self.ws.data_ptr()), self.ws.numel(),
                                         _stream() if stream is None else stream)
        L.check(st, "cloud_points")

    def check(self, pattern=None):
        """every byte against the restatement of `pattern` (the object's own if None)"""
        B, h, w = self.shape
        bodies, counts, maps, rec = R.want(self.shape, pattern or self.pattern, self.form)
        what = (self.shape, pattern or self.pattern, self.form)
        torch.cuda.synchronize()
        assert rec == self.rec and np.array_equal(self.counts.cpu().numpy().view(np.uint32), counts), (what, self.counts.tolist())
        got = self.body.cpu().numpy()
        assert got[0] == FILL and got[-1] == FILL, (what, "a byte outside the body was written")
        got = got[1:-1].reshape(B, h * w * rec)
        for b, body in enumerate(bodies):
            want = np.frombuffer(body, dtype=np.uint8)
            bad = np.flatnonzero(got[b, :len(want)] != want)
            assert bad.size == 0, f"{what} image {b}: {bad.size} bytes differ, the first in record {bad[0] // rec} at byte {bad[0] % rec}"
            assert (got[b, len(want):] == FILL).all(), (what, b, "bytes behind the records were written")
        if self.nmap:
            m = self.map.cpu().numpy()
            assert m[0] == FILL and m[-1] == FILL and np.array_equal(m[1:-1].reshape(maps.shape), maps), (what, "normal map")
        assert self.codes_buf[0] == 1 and self.codes_buf[-1] == 1


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_equals_the_restatement(shape):
    """cloud_ref.cases: every pattern under every record form -- the four forms, grey and RGB, R = 1, 2 and 8, A = 0, with and
    without the normal map; u8, u16 and codes of 32768 and above"""
    for pattern, form in R.cases(shape):
        case = Raw(shape, pattern, form)
        case.run()
        case.check()


def test_what_the_case_set_covers():
    """From the restatement: count 0 and count 1 occur; normals are found and refused in one case; the spans of the blocks of one
    case start at all four addresses modulo 4 for an odd record; the scan's threads take more than one word on the largest plane"""
    assert R.want(R.SHAPES[3], "none", "full")[1].tolist() == [[0, 0]] and R.want(R.SHAPES[4], "last", "full")[1].tolist() == [[1, 0]]
    pts, nrm = R.want(R.SHAPES[6], "random", "full")[1][0]
    assert 0 < nrm < pts
    c = R.plane(R.SHAPES[6], "random")[0].ravel() != 0
    starts = np.concatenate([[0], np.cumsum([c[q:q + R.RUN].sum() for q in range(0, c.size, R.RUN)])[:-1]])
    assert {int((1 + s * 27) % 4) for s in starts} == {0, 1, 2, 3}
    assert -(-R.BIG[1] * R.BIG[2] // R.RUN) == 260 > 256
    assert {f[1:3] for f in R.FORMS} >= {(False, 0), (True, 0), (False, 1), (True, 3), (True, 1)}


def test_a_second_call_two_streams_and_the_python_interface():
    """The workspace is initialised by every call: a second call on the same stream and buffers with other codes equals its own
    restatement.  Two streams, a workspace each.  Unprojection gives the same bytes, for (h, w) planes and uint16 tensors too."""
    shape = R.SHAPES[6]
    case = Raw(shape, "all", "full")
    case.run()
    case.check()
    for pattern in ("random", "none", "checker", "random"):
        case.codes.copy_(torch.from_numpy(np.array(R.plane(shape, pattern)).view(np.int16)).cuda())
        case.body.fill_(FILL)
        case.run()
        case.check(pattern)
    torch.cuda.synchronize()
    un = K.Unprojection(P.Camera(shape[2], shape[1], *R.camera_of(shape)), tolerance=20)
    assert np.array_equal(un.rx.cpu().numpy(), R.tables(shape)[0]) and np.array_equal(un.ry.cpu().numpy(), R.tables(shape)[1])
    outs = []
    for stream, pattern, tinted in zip((torch.cuda.Stream(), torch.cuda.Stream()), ("random", "surfaces"), (True, False)):
        with torch.cuda.stream(stream):
            codes = torch.from_numpy(np.array(R.plane(shape, pattern)).view(np.int16)).cuda()
            color = torch.from_numpy(np.array(R.tint(shape, 3))).cuda() if tinted else None
            outs.append((un(codes, color, 10000, normal_map=True), pattern, "full" if tinted else "normals"))
    torch.cuda.synchronize()
    for got, pattern, form in outs:
        bodies, counts, maps, rec = R.want(shape, pattern, form)
        assert got.rec == rec and got.body.shape == (1, shape[1] * shape[2] * rec) and got.counts.dtype == torch.int32
        assert np.array_equal(got.counts.cpu().numpy().view(np.uint32), counts)
        assert got.body[0, :len(bodies[0])].cpu().numpy().tobytes() == bodies[0]
        assert np.array_equal(got.normal_map.cpu().numpy(), maps)
    codes = torch.from_numpy(np.array(R.plane(shape, "random")).view(np.int16)).cuda()
    one = un(codes[0], depth_max=10000)
    u16 = un(codes.view(torch.uint16), depth_max=10000)
    bodies, counts, _, rec = R.want(shape, "random", "normals")
    for got in (one, u16):
        assert got.normal_map is None and got.rec == 24 and got.body[0, :len(bodies[0])].cpu().numpy().tobytes() == bodies[0]
    grey = K.Unprojection(P.Camera(shape[2], shape[1], *R.camera_of(shape)), normals=False)(codes, torch.from_numpy(np.array(R.tint(shape, 1))).cuda())
    assert grey.rec == 15 and grey.body[0, :len(R.want(shape, "random", "grey")[0][0])].cpu().numpy().tobytes() == R.want(shape, "random", "grey")[0][0]
    with pytest.raises(RuntimeError, match="cloud_points expects"):
        un(codes.float())
    with pytest.raises(ValueError, match="cloud_points: a 5x7 plane, and the camera is 93x116"):
        un(codes[0, :5, :7])
    with pytest.raises(ValueError, match="cloud_points: tolerance 20 above the largest code 5"):
        un(codes, depth_max=5)
    with pytest.raises(RuntimeError, match="cloud_points expects color as uint8"):
        un(codes, torch.zeros((1, 93, 116, 4), dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="cloud_points expects color as uint8"):
        un(codes, torch.zeros((1, 93, 116), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="a normal map without normals"):
        K.Unprojection(P.Camera(shape[2], shape[1], *R.camera_of(shape)), normals=False)(codes, normal_map=True)


def test_capture_and_replay():
    """One call inside a capture (a single branch: three launches in a row on the capture's stream) and one replay on changed
    contents of the same input equal the restatement of the changed contents"""
    shape = R.SHAPES[6]
    case = Raw(shape, "checker", "full")
    case.run()                                                        # eager first: every allocation exists before the capture
    case.check()
    case.body.fill_(FILL)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        case.run(stream=ops._stream(torch.device("cuda:0")))
    case.codes.copy_(torch.from_numpy(np.array(R.plane(shape, "random")).view(np.int16)).cuda())
    case.body.fill_(FILL)
    graph.replay()
    case.check("random")


def test_refusals_leave_every_output_untouched():
    lib = L.load()
    shape = R.SHAPES[2]
    case = Raw(shape, "random", "abs_0")                              # the good call's form: normals, RGB, no map
    keep = case.codes_buf.clone()
    call = cloud_caller(lib, case.codes.data_ptr(), case.rx.data_ptr(), case.ry.data_ptr(), case.body.data_ptr() + 1,
                        case.counts.data_ptr(), case.ws.data_ptr(), color=case.color.data_ptr(), stream=_stream())
    cloud_refusals(lib, call)
    assert "unaligned" in call(src=case.codes.data_ptr() + 1)[1] and "unaligned" in call(ws=case.ws.data_ptr() + 8)[1]
    assert "unaligned" in call(counts=case.counts.data_ptr() + 2)[1] and "unaligned" in call(rx=case.rx.data_ptr() + 1)[1]
    torch.cuda.synchronize()
    assert (case.body == FILL).all() and (case.counts == -7).all() and torch.equal(case.codes_buf, keep)
    rx, ry = R.tables(shape)
    st, msg = call(span=(int(rx[0]), int(rx[-1]), int(ry[0]), int(ry[-1])), tol_abs=0, top=10000)           # and the good call goes through
    assert st == 0, msg
    case.check()


# ---- the command lines -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_writes_what_read_ply_reads(tmp_path, capsys, bits, top):
    """cloud.main on three files: the PLY files equal the restatement, with colour (RGB, grey, and a larger image cropped), the
    normal maps as RGB PNGs, the statistics lines; --camera depth, --no-normals and --scale on the same files"""
    from PIL import Image
    h, w = 37, 52
    color_cam = dict(width=w, height=h, fx=61.5, fy=60.25, cx=25.25, cy=18.5)
    depth_cam = dict(width=w, height=h, fx=58.0, fy=57.0, cx=26.0, cy=17.75, dist=[0.0] * 5)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps({"depth": depth_cam, "color": color_cam, "rotation": np.eye(3).tolist(), "translation": [0.0, 0.0, 0.0]}))
    depth, color, out, maps = (str(tmp_path / n) for n in ("depth", "color", "out", "maps"))
    os.makedirs(depth), os.makedirs(color)
    write = io.write_gray if bits == 8 else io.write_depth16
    g = np.random.default_rng(11)
    planes, tints = [], []
    for i, pattern in enumerate(("u8" if bits == 8 else "random", "surfaces", "checker")):
        c = R.plane((1, h, w), pattern)[0]
        c = np.clip(c, 0, top).astype(np.uint8 if bits == 8 else np.uint16)
        write(os.path.join(depth, f"{i:02d}.png"), c)
        rgb = g.integers(0, 256, size=(h + (i == 2), w + 2 * (i == 2), 3), dtype=np.uint8)       # the third is larger: cropped
        if i == 1:
            rgb = rgb[..., 0]
            io.write_gray(os.path.join(color, f"{i:02d}.png"), rgb)
        else:
            Image.fromarray(rgb, mode="RGB").save(os.path.join(color, f"{i:02d}.png"))
        planes.append(c), tints.append(rgb[:h, :w])
    fmt = ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []
    A = max(2, top // 500)
    capsys.readouterr()
    assert K.main(["--depth", depth, "--calib", str(rig), "--out", out, "--color", color, "--normal-maps", maps, "--stats",
                   "--normal-tolerance", str(A), *fmt]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    rx, ry = R.ray_tables(w, h, color_cam["fx"], color_cam["fy"], color_cam["cx"], color_cam["cy"])
    for i, (c, rgb) in enumerate(zip(planes, tints)):
        rec, counts, nmap = R.cloud_plane(c, rx, ry, tolerance=A, color=rgb)
        got = K.read_ply(os.path.join(out, f"{i:02d}.ply"))
        assert got.dtype == rec.dtype and got.tobytes() == rec.tobytes(), i
        assert lines[i] == f"{i:02d}.png points={counts[0]} normals={counts[1]}"
        assert np.array_equal(np.asarray(Image.open(os.path.join(maps, f"{i:02d}.png")).convert("RGB")), nmap), i
    # the depth camera's own frame, positions alone, no statistics
    plain = str(tmp_path / "plain")
    assert K.main(["--depth", depth, "--calib", str(rig), "--out", plain, "--camera", "depth", "--no-normals", "--depth-unit", "0.0005",
                   *fmt]) == 0
    assert capsys.readouterr().out.strip().splitlines() == ["00.png", "01.png", "02.png"]
    dx, dy = R.ray_tables(w, h, depth_cam["fx"], depth_cam["fy"], depth_cam["cx"], depth_cam["cy"])
    for i, c in enumerate(planes):
        rec, _, _ = R.cloud_plane(c, dx, dy, depth_unit=0.0005, normals=False)
        assert K.read_ply(os.path.join(plain, f"{i:02d}.ply")).tobytes() == rec.tobytes(), i
    # the same files read as maps on a four times larger colour grid: the camera is projection_q8's
    big = tmp_path / "big.json"
    big_cam = dict(width=4 * w + 3, height=4 * h + 1, fx=246.0, fy=241.0, cx=101.5, cy=75.5)
    big.write_text(json.dumps({"depth": depth_cam, "color": big_cam, "rotation": np.eye(3).tolist(), "translation": [0.0, 0.0, 0.0]}))
    quarter = str(tmp_path / "quarter")
    assert K.main(["--depth", depth, "--calib", str(big), "--out", quarter, "--scale", "4", "--normal-radius", "1",
                   "--normal-tolerance", str(A), *fmt]) == 0
    qx, qy = R.ray_tables(w, h, 246.0 / 4, 241.0 / 4, (101.5 + 0.5) / 4 - 0.5, (75.5 + 0.5) / 4 - 0.5)
    for i, c in enumerate(planes):
        rec, _, _ = R.cloud_plane(c, qx, qy, radius=1, tolerance=A)
        assert K.read_ply(os.path.join(quarter, f"{i:02d}.ply")).tobytes() == rec.tobytes(), i
    # a colour image smaller than the map is refused by name
    Image.fromarray(np.zeros((h - 1, w, 3), dtype=np.uint8), mode="RGB").save(os.path.join(color, "00.png"))
    with pytest.raises(ValueError, match=f"00.png: {h - 1}x{w}, smaller than the {h}x{w}"):
        K.main(["--depth", depth, "--calib", str(rig), "--out", out, "--color", color, *fmt])


def test_register_infer_cloud_run_through(tmp_path, capsys):
    """register.main -> infer --lr-depth --baseline bicubic --fill-holes -> cloud.main on three files: the clouds are the
    restatement of the super-resolved maps under the colour camera"""
    shape = G.SHAPES[5]                                               # 70 x 130 onto 35 x 65 at scale 4 of 140 x 260
    hs, ws = shape[1:3]
    top = 10000
    m = G.calibration(shape, "mixed")
    sensor, lr, sr, color, out = (str(tmp_path / n) for n in ("sensor", "lr", "sr", "color", "out"))
    os.makedirs(sensor), os.makedirs(color)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(m))
    g = np.random.default_rng(5)
    for i in range(3):
        io.write_depth16(os.path.join(sensor, f"{i:02d}.png"), G.plane(shape, ("random", "scene", "random")[i], top, seed=1 + i)[0])
        io.write_gray(os.path.join(color, f"{i:02d}.png"), g.integers(0, 256, size=(140, 260), dtype=np.uint8))
    fmt = ["--depth-bits", "16", "--depth-max", str(top)]
    unit = repr(G.unit_of(top))
    assert P.main(["--depth", sensor, "--calib", str(rig), "--out", lr, "--scale", "4", "--depth-unit", unit, *fmt]) == 0
    assert infer.main(["--scale", "4", "--lr-depth", lr, "--input-color", color, "--out", sr, "--baseline", "bicubic", "--fill-holes",
                       *fmt]) == 0
    capsys.readouterr()
    assert K.main(["--depth", sr, "--calib", str(rig), "--out", out, "--color", color, "--depth-unit", unit, "--stats", *fmt]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    cam = m["color"]
    rx, ry = R.ray_tables(cam["width"], cam["height"], cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    total = 0
    for i in range(3):
        c = io.read_depth_plane(os.path.join(sr, f"{i:02d}.png"), 16, top)
        assert c.shape == (140, 260)
        rec, counts, _ = R.cloud_plane(c, rx, ry, depth_unit=G.unit_of(top), color=io.read_gray(os.path.join(color, f"{i:02d}.png")))
        got = K.read_ply(os.path.join(out, f"{i:02d}.ply"))
        assert len(got) == counts[0] and got.tobytes() == rec.tobytes(), i
        assert lines[i] == f"{i:02d}.png points={counts[0]} normals={counts[1]}"
        total += int(counts[0])
    assert total > 0
