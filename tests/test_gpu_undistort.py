"""The undistortion of colour images on the MI355X against the numpy restatement tests/undistort_ref.py (pinned on the
CPU by tests/test_undistort_cpu.py).  The bar is EQUAL BITS everywhere, no tolerance.
Shapes (undistort_ref.SHAPES), the smallest at which each part can go wrong: one grey pixel (every tap clamps); 7 x 9 RGB, less than
a tile; exactly one 32 x 8 tile with both channel counts; 9 x 33 in a batch of three, one past a tile on both axes; 40 x 100, several
tiles, with both channel counts; 40 x 100 onto 24 x 50, an output camera of another size.  Rigs: identity, barrel, pincushion
(outside pixels and EMPTY tiles), zoom-out (STAGED, DIRECT and EMPTY tiles in one call), a principal point half an image aside.
Patterns: noise, constant 255, a ramp."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops
from codon_amd import register as P
from codon_amd import undistort as D
from tests import register_ref as G
from tests import undistort_ref as U
from tests.test_undistort_cpu import undistort_caller, undistort_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731
P_ = C.c_void_p


def _camera(t):
    w, h, fx, fy, cx, cy, dist = t
    return P.Camera(w, h, fx, fy, cx, cy, dist)


def _und(shape, rig):
    src, dst = U.cameras(shape, rig)
    return D.Undistortion(_camera(src), _camera(dst))


def _form(a, C_):
    """the restatement's (B, H, W, C) as the module takes and returns it: (B, H, W) grey, (B, H, W, 3) RGB"""
    return a if C_ == 3 else a[..., 0]


@pytest.mark.parametrize("shape", U.SHAPES, ids=ids)
def test_equals_the_restatement(shape):
    """undistort_ref.cases: every rig under every pattern -- the tables, the counts, every byte; the argument is not modified; a
    single image without the batch dimension gives the batch's first"""
    B, H, W, C_, ho, wo = shape
    for rig in U.RIGS:
        und = _und(shape, rig)
        M, tiles, counts = U.tables(shape, rig)
        assert np.array_equal(und.map.cpu().numpy(), M) and np.array_equal(und.tiles.cpu().numpy(), tiles)
        assert np.array_equal(und.weights.cpu().numpy(), U.weight_table())
        assert und.counts == dict(zip(U.COUNTS, (int(v) for v in counts)))
        assert (und.dst.height, und.dst.width) == (ho, wo)
        for pattern in U.PATTERNS:
            want = _form(U.want(shape, rig, pattern), C_)
            src = torch.from_numpy(_form(U.image(shape, pattern), C_).copy()).cuda()
            before = src.clone()
            got = und(src, C_)
            assert got.shape == want.shape and got.dtype == torch.uint8 and got.is_contiguous()
            bad = np.argwhere(got.cpu().numpy() != want)
            assert bad.size == 0, f"{shape} {rig} {pattern}: {len(bad)} bytes differ, first at {bad[:3].tolist()}"
            assert torch.equal(src, before)
            one = und(src[0], C_)
            assert one.shape == want.shape[1:] and np.array_equal(one.cpu().numpy(), want[0])


def test_the_case_set_reaches_every_part():
    """Conditions over the case set, from .counts and the restatement: the three tile kinds occur, and in ONE call under the zoom-out
    rig; outside pixels occur; the noise cases hold results the clamp raised to 0 and lowered to 255"""
    total = dict.fromkeys(U.COUNTS, 0)
    low = high = 0
    for shape in U.SHAPES:
        for rig in U.RIGS:
            c = _und(shape, rig).counts
            for k in U.COUNTS:
                total[k] += c[k]
            lo, hi = U.clamped(U.image(shape, "noise"), U.tables(shape, rig)[0])
            low, high = low + lo, high + hi
    assert total["staged"] > 0 and total["direct"] > 0 and total["empty"] > 0 and total["outside"] > 0, total
    assert low > 0 and high > 0
    c = _und(U.SHAPES[6], "zoom_out").counts
    assert (c["staged"], c["direct"], c["empty"]) == (10, 3, 7)
    c = _und(U.SHAPES[6], "pincushion").counts
    assert c["outside"] > 0 and c["empty"] > 0
    assert min(U.clamped(U.image(U.SHAPES[6], "noise"), U.tables(U.SHAPES[6], "barrel")[0])) > 0


def _call(lib, und, B, shape, src_ptr, out_ptr):
    _, H, W, C_, ho, wo = shape
    return lib.codon_undistort(B, H, W, C_, P_(src_ptr), ho, wo, P_(und.map.data_ptr()), P_(und.tiles.data_ptr()),
                               P_(und.weights.data_ptr()), P_(out_ptr), ops._stream(torch.device("cuda:0")))


@pytest.mark.parametrize("shape", [U.SHAPES[4], U.SHAPES[7]], ids=ids)
def test_unaligned_views(shape):
    """in and out one byte into larger buffers: no alignment is promised for either; the bytes around out stay"""
    lib = L.load()
    B, H, W, C_, ho, wo = shape
    und = _und(shape, "zoom_out")
    img = U.image(shape, "noise")
    n_in, n_out = img.size, B * ho * wo * C_
    src = torch.zeros(n_in + 2, dtype=torch.uint8, device="cuda")
    src[1:1 + n_in] = torch.from_numpy(img.reshape(-1)).cuda()
    out = torch.full((n_out + 2,), 0xEE, dtype=torch.uint8, device="cuda")
    assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
    assert _call(lib, und, B, shape, src.data_ptr() + 1, out.data_ptr() + 1) == 0, lib.codon_last_error_string()
    got = out.cpu().numpy()
    assert got[0] == 0xEE and got[-1] == 0xEE
    assert np.array_equal(got[1:-1].reshape(B, ho, wo, C_), U.want(shape, "zoom_out", "noise"))
    # and through the module: a contiguous view at an odd address
    view = src[1:1 + n_in].view(B, H, W, C_)
    assert view.data_ptr() % 2 == 1
    assert np.array_equal(und(_form(view, C_), C_).cpu().numpy(), _form(U.want(shape, "zoom_out", "noise"), C_))


def test_a_second_call_and_two_streams():
    shape = U.SHAPES[6]
    und = _und(shape, "zoom_out")
    first = und(torch.from_numpy(U.image(shape, "white")).cuda(), 3)
    for pattern in ("noise", "ramp", "white"):
        got = und(torch.from_numpy(U.image(shape, pattern)).cuda(), 3)
        assert np.array_equal(got.cpu().numpy(), U.want(shape, "zoom_out", pattern)), pattern
    assert torch.equal(got, first)
    dev = torch.from_numpy(U.image(shape, "noise")).cuda()
    torch.cuda.synchronize()
    outs = []
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            outs.append(und(dev, 3))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and np.array_equal(outs[0].cpu().numpy(), U.want(shape, "zoom_out", "noise"))


def test_capture_and_replay():
    """One call inside a capture (a single branch: one launch) and one replay on other contents of the same input tensor"""
    shape = U.SHAPES[7]
    und = _und(shape, "barrel")
    a, b = torch.from_numpy(U.image(shape, "noise")).cuda(), torch.from_numpy(U.image(shape, "ramp")).cuda()
    src = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = und(src, 3)
    src.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), U.want(shape, "barrel", "ramp"))


def test_refusals_leave_out_untouched():
    lib = L.load()
    cam = P.Camera(7, 5, 4.2, 4.3, 3.37, 1.81, U.BARREL)
    und = D.Undistortion(cam)
    src = torch.from_numpy(np.random.default_rng(1).integers(0, 256, size=(5, 7), dtype=np.uint8)).cuda()
    out = torch.full((2, 5, 7), 0xEE, dtype=torch.uint8, device="cuda")
    keep = src.clone()
    call = undistort_caller(lib, src.data_ptr(), und.map.data_ptr(), und.tiles.data_ptr(), und.weights.data_ptr(), out.data_ptr(),
                            ops._stream(torch.device("cuda:0")))
    undistort_refusals(lib, call)
    torch.cuda.synchronize()
    assert (out == 0xEE).all() and torch.equal(src, keep)
    assert call()[0] == 0                                                # and the good call goes through
    torch.cuda.synchronize()
    M = U.map_table((7, 5, 4.2, 4.3, 3.37, 1.81, U.BARREL), (7, 5, 4.2, 4.3, 3.37, 1.81, (0.0,) * 5))
    assert np.array_equal(out[0].cpu().numpy(), U.undistort(keep.cpu().numpy()[None, :, :, None], M)[0, :, :, 0])
    assert (out[1] == 0xEE).all()
    with pytest.raises(RuntimeError, match="the image on cuda:0, the tables on cpu"):
        D.Undistortion(cam, device="cpu")(src)


# ---- the command line, then register and infer on what it wrote ---------------------------------------------------------------------------

def test_main_then_register_then_infer(tmp_path, capsys):
    """undistort.main on three files (two RGB, one grey) writes PNGs equal to the restatement, prints the counts and writes the
    rectified calibration; register.main refuses the rig's own file and accepts that one; infer --lr-depth --baseline jbu
    --fill-holes --fill-guided then runs on what both wrote: the chain, with no network needed"""
    from PIL import Image
    shape, top = G.SHAPES[5], 255                                        # a sensor onto a 140 x 260 colour image at scale 4
    rig = G.calibration(shape, "mixed")
    rig["color"]["dist"] = list(U.BARREL)
    rig["serial"] = "A17"
    c = rig["color"]
    src = (c["width"], c["height"], c["fx"], c["fy"], c["cx"], c["cy"], tuple(c["dist"]))
    assert (c["height"], c["width"]) == (140, 260)
    dst = U.out_camera(src, 0.9)
    M = U.map_table(src, dst)
    counts = U.tile_table(M)[1]
    sensor, color, flat, lr, sr = (str(tmp_path / n) for n in ("sensor", "color", "flat", "lr", "sr"))
    os.makedirs(sensor), os.makedirs(color)
    (tmp_path / "rig.json").write_text(json.dumps(rig))
    g = np.random.default_rng(5)
    pics = []
    for i, pattern in enumerate(("random", "scene", "none")):
        io.write_gray(os.path.join(sensor, f"{i:02d}.png"), G.plane(shape, pattern, top, seed=2 + i)[0])
        yy, xx = np.mgrid[0:140, 0:260]
        pic = (96 + 64 * np.sin(0.05 * xx[..., None] + np.arange(3)) * np.cos(0.07 * yy[..., None]) + g.integers(0, 32, size=(140, 260, 3)))
        pic = pic.astype(np.uint8) if i < 2 else pic.astype(np.uint8)[..., 1]
        Image.fromarray(pic, mode="RGB" if i < 2 else "L").save(os.path.join(color, f"{i:02d}.png"))
        pics.append(pic)
    argv = ["--color", color, "--calib", str(tmp_path / "rig.json"), "--out", flat, "--focal-scale", "0.9"]
    capsys.readouterr()
    assert D.main(argv + ["--calib-out", str(tmp_path / "rect.json"), "--stats"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    s, d, e, o = (int(v) for v in counts)
    assert lines == [f"{i:02d}.png outside={o} staged={s} direct={d} empty={e}" for i in range(3)] and o > 0
    for i, pic in enumerate(pics):
        im = Image.open(os.path.join(flat, f"{i:02d}.png"))
        assert im.mode == ("RGB" if i < 2 else "L")
        want = U.undistort(pic.reshape(1, 140, 260, -1), M)[0]
        assert np.array_equal(np.asarray(im).reshape(want.shape), want), i
    rect = json.loads((tmp_path / "rect.json").read_text())
    assert rect["color"] == {"width": 260, "height": 140, "fx": dst[2], "fy": dst[3], "cx": dst[4], "cy": dst[5], "dist": [0.0] * 5}
    assert {k: v for k, v in rect.items() if k != "color"} == {k: v for k, v in rig.items() if k != "color"}
    # --gray converts first and writes grey
    assert D.main(argv + ["--out", str(tmp_path / "gray"), "--gray"]) == 0
    assert capsys.readouterr().out.strip().splitlines() == ["00.png", "01.png", "02.png"]
    im = Image.open(tmp_path / "gray" / "00.png")
    grey = io.read_gray(os.path.join(color, "00.png"))
    assert im.mode == "L" and np.array_equal(np.asarray(im), U.undistort(grey[None, :, :, None], M)[0, :, :, 0])
    # an image of another size is refused by name
    other = tmp_path / "other"
    other.mkdir()
    io.write_gray(str(other / "a.png"), np.zeros((140, 259), dtype=np.uint8))
    with pytest.raises(SystemExit, match="a.png: a 140x259 image, and the colour camera of the calibration is 140x260"):
        D.main(["--color", str(other), "--calib", str(tmp_path / "rig.json"), "--out", str(tmp_path / "o2")])
    # register: the rig's own file is refused, the rectified one registers onto the grid the images now have
    reg = ["--depth", sensor, "--out", lr, "--scale", "4", "--depth-unit", repr(G.unit_of(top))]
    with pytest.raises(SystemExit) as ex:
        P.main(reg + ["--calib", str(tmp_path / "rig.json")])
    assert ex.value.code == 2 and "undistort the colour images first (python -m codon_amd.undistort" in capsys.readouterr().err
    assert P.main(reg + ["--calib", str(tmp_path / "rect.json")]) == 0
    cal = P.Calibration.from_mapping(rect)
    assert cal.color == _camera(dst)
    A, T, Q = P.ray_table(cal), P.translation_q20(cal, G.unit_of(top)), P.projection_q8(cal, 4)
    for i, pattern in enumerate(("random", "scene", "none")):
        want = G.register_plane(G.plane(shape, pattern, top, seed=2 + i)[0], A, T, Q, 35, 65, top)[0]
        assert np.array_equal(io.read_depth_plane(os.path.join(lr, f"{i:02d}.png"), 8), want), i
    rc = infer.main(["--scale", "4", "--lr-depth", lr, "--input-color", flat, "--out", sr, "--baseline", "jbu", "--fill-holes",
                     "--fill-guided"])
    assert rc == 0
    up = io.read_depth_plane(os.path.join(sr, "01.png"), 8)
    assert up.shape == (140, 260) and (up != 0).all()
