"""The undistortion's definition (tests/undistort_ref.py) on the CPU: what the definition promises -- identity, exact
shifts, constants, the fold rule, the accuracy of the resampling on a ramp against a bound computed from the tables -- the host
tables of codon_amd.undistort against the restatement's, the host's tile table (codon_undistort_plan) against the restatement's, and
every refusal that needs no GPU: of the C entries (validated on the host before any HIP call), of the module and of the command
line, and the hand-over of the rectified calibration to codon_amd.register.  Expectations are spelled out here, not derived from
the code under test."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import register as P
from codon_amd import undistort as D
from tests import undistort_ref as U

P_ = C.c_void_p


def _camera(t):
    w, h, fx, fy, cx, cy, dist = t
    return P.Camera(w, h, fx, fy, cx, cy, dist)


def _plan(lib, hs, ws, M):
    """codon_undistort_plan on a host map -> (status, message, tiles, counts)"""
    M = np.ascontiguousarray(M, dtype=np.int32)
    ho, wo = M.shape[:2]
    tiles = np.full(lib.codon_undistort_tiles_bytes(ho, wo) // 4, -77, dtype=np.int32)
    counts = np.full(4, 77, dtype=np.uint32)
    st = lib.codon_undistort_plan(hs, ws, ho, wo, P_(M.ctypes.data), P_(tiles.ctypes.data), P_(counts.ctypes.data))
    return st, lib.codon_last_error_string().decode(), tiles.reshape(-(-ho // 8), -(-wo // 32), 4), counts


# ---- the tables -------------------------------------------------------------------------------------------------------------------------

def test_the_host_tables_are_the_restatement():
    K = D.weight_table()
    assert K.dtype == np.int16 and K.shape == (32, 4) and np.array_equal(K, U.weight_table())
    assert (K.astype(np.int64).sum(axis=1) == 2048).all()
    assert K[0].tolist() == [0, 2048, 0, 0] and K[16].tolist() == [-128, 1152, 1152, -128]
    for shape in U.SHAPES:
        for rig in U.RIGS:
            src, dst = U.cameras(shape, rig)
            M = D.map_table(_camera(src), _camera(dst))
            assert M.dtype == np.int32 and M.shape == (shape[4], shape[5], 2)
            assert np.array_equal(M, U.tables(shape, rig)[0]), (shape, rig)
            inside = M[..., 0] != U.OUTSIDE
            assert (M[~inside] == U.OUTSIDE).all()
            assert (M[inside] >= -16).all() and (M[inside][:, 0] < 32 * shape[2] - 16).all() and (M[inside][:, 1] < 32 * shape[1] - 16).all()
    cam = _camera(U.cameras(U.SHAPES[5], "barrel")[0])
    out = D.out_camera(cam, 0.5)
    assert out == P.Camera(100, 40, cam.fx * 0.5, cam.fy * 0.5, cam.cx, cam.cy) and not any(out.dist)
    assert D.out_camera(cam) == P.Camera(100, 40, cam.fx, cam.fy, cam.cx, cam.cy)
    assert D.r2_fold((0.0,) * 5) == np.inf and D.r2_fold(U.PINCUSHION) == np.inf
    assert D.r2_fold((-0.3, 0, 0, 0, 0)) == 4552 / 4096                  # 1 - 0.9 rho <= 0 from rho = 1.1111: n = 4552
    with pytest.raises(ValueError, match="map_table: dst.dist"):
        D.map_table(cam, cam)
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="out_camera: focal_scale"):
            D.out_camera(cam, bad)


def test_the_int32_bound_from_the_table():
    """row_r is at most 255 max sum |K[p]| in magnitude and acc at most that times max sum |K[p]|; with the rounding constant the
    largest intermediate stays below 2^31"""
    s = int(np.abs(D.weight_table().astype(np.int64)).sum(axis=1).max())
    assert s == 2560
    assert 255 * s * s + (1 << 21) == 1673265152 < (1 << 31)


# ---- what the definition promises --------------------------------------------------------------------------------------------------------

NON_DYADIC = dict(fx=57.3, fy=61.9, cx=15.37, cy=11.81)


def test_identity_returns_the_image():
    """Zero distortion and one camera in both roles: a random RGB image comes back bit for bit, for non-dyadic intrinsics"""
    cam = P.Camera(32, 24, **NON_DYADIC)
    M = D.map_table(cam, D.out_camera(cam))
    j, i = np.meshgrid(np.arange(32), np.arange(24))
    assert np.array_equal(M[..., 0], 32 * j) and np.array_equal(M[..., 1], 32 * i)
    img = np.random.default_rng(3).integers(0, 256, size=(2, 24, 32, 3), dtype=np.uint8)
    assert np.array_equal(U.undistort(img, M, D.weight_table()), img)


def test_a_principal_point_shift_is_an_exact_shift():
    """The output camera's principal point moved by (+7, -3) whole pixels: out[i][j] = img[i + 3][j - 7], and the pixels whose source
    lies outside the image are 0: 7 columns and 3 rows, 3 W + 7 H - 21 of them"""
    H, W = 24, 32
    cam = P.Camera(W, H, **NON_DYADIC)
    dst = P.Camera(W, H, cam.fx, cam.fy, cam.cx + 7, cam.cy - 3)
    M = D.map_table(cam, dst)
    _, msg, _, counts = _plan(L.load(), H, W, M)
    assert counts[3] == 3 * W + 7 * H - 21 == int((M[..., 0] == U.OUTSIDE).sum()), msg
    img = np.random.default_rng(4).integers(1, 256, size=(1, H, W, 3), dtype=np.uint8)
    want = np.zeros_like(img)
    want[:, :H - 3, 7:] = img[:, 3:, :W - 7]
    assert np.array_equal(U.undistort(img, M, D.weight_table()), want)


@pytest.mark.parametrize("rig", ["barrel", "pincushion", "zoom_out"])
def test_a_constant_image_stays_constant(rig):
    shape = U.SHAPES[6]
    M = U.tables(shape, rig)[0]
    for v in (0, 1, 127, 255):
        out = U.undistort(np.full(shape[:4], v, dtype=np.uint8), M, D.weight_table())
        inside = M[..., 0] != U.OUTSIDE
        assert inside.any() and (out[:, inside] == v).all() and (out[:, ~inside] == 0).all()


def test_the_fold_rule():
    """A 40 x 100 image with f = 60 and k1 = -0.3, seen by an output camera of 0.4 times the focal length: most of the pixels whose
    source position passes the box test lie beyond the radius 1.111 at which r (1 - 0.3 r^2) turns back, and would show a mirrored
    ghost of the image; the rule makes them outside"""
    src = (100, 40, 60.0, 60.0, 49.5, 19.5, (-0.3, 0.0, 0.0, 0.0, 0.0))
    dst = U.out_camera(src, 0.4)
    box = U.map_table(src, dst, fold=False)[..., 0] != U.OUTSIDE
    M = D.map_table(_camera(src), D.out_camera(_camera(src), 0.4))
    assert np.array_equal(M, U.map_table(src, dst))
    inside = M[..., 0] != U.OUTSIDE
    assert not (inside & ~box).any()
    assert int(box.sum()) == 2908 and int((box & ~inside).sum()) == 1988
    j, i = np.meshgrid(np.arange(100.0), np.arange(40.0))
    r2 = ((j - 49.5) / 24.0) ** 2 + ((i - 19.5) / 24.0) ** 2              # spelled out: the normalised radius of the target pixel
    assert np.array_equal(inside, box & (r2 < 4552 / 4096))


def test_accuracy_on_a_ramp():
    """A linear ramp a x + b y + c rounded to u8 through the barrel rig, against the exact a u + b v + c at the float64 source
    position, over the pixels whose 4 x 4 footprint is interior and unsaturated.  The bound, from the tables: the 16 rounded taps
    err by at most 0.5 each, weighted by at most (max sum |K| / 2048)^2; the position is rounded to 1 / 32 pixel, at most 1 / 64
    on either axis; the output is rounded, 0.5; and a row of K misses the first moment of its phase by at most m pixels, on either
    axis (a cubic through a linear ramp is otherwise exact: every row sums to 2048)."""
    a, b, c = 1.7, -2.3, 120.0
    shape = U.SHAPES[5]
    H, W = shape[1:3]
    src, dst = U.cameras(shape, "barrel")
    j, i = np.meshgrid(np.arange(W, dtype=np.float64), np.arange(H, dtype=np.float64))
    exact = a * j + b * i + c
    img = np.clip(np.rint(exact), 0, 255).astype(np.uint8)[None, :, :, None]
    K = D.weight_table().astype(np.float64)
    M = D.map_table(_camera(src), _camera(dst))
    out = U.undistort(img, M, D.weight_table())[0, :, :, 0].astype(np.float64)
    x, y = (j - dst[4]) / dst[2], (i - dst[5]) / dst[3]
    xd, yd = P.distort(x, y, src[6])
    u, v = src[2] * xd + src[4], src[3] * yd + src[5]
    xi, yi = M[..., 0] >> 5, M[..., 1] >> 5
    ok = (M[..., 0] != U.OUTSIDE) & (xi >= 1) & (xi + 2 <= W - 1) & (yi >= 1) & (yi + 2 <= H - 1)
    corners = [a * (xi + dx) + b * (yi + dy) + c for dx in (-1, 2) for dy in (-1, 2)]
    ok &= (np.min(corners, axis=0) >= 0.5) & (np.max(corners, axis=0) <= 254.5)
    m = np.abs((K * np.array([-1.0, 0.0, 1.0, 2.0])).sum(axis=1) / 2048.0 - np.arange(32) / 32.0).max()
    bound = 0.5 * (np.abs(K).sum(axis=1).max() / 2048.0) ** 2 + (abs(a) + abs(b)) / 64.0 + 0.5 + (abs(a) + abs(b)) * m
    err = np.abs(out - (a * u + b * v + c))[ok]
    print(f"accuracy: {int(ok.sum())} pixels, largest error {err.max():.4f}, bound {bound:.4f}, first-moment error {m:.2e}")
    assert ok.sum() > 1000 and 1.0 < bound < 1.5
    assert err.max() <= bound


# ---- the tile table: the C entry on the host -----------------------------------------------------------------------------------------------

def test_plan_is_the_restatement():
    lib = L.load()
    assert lib.codon_undistort_tiles_bytes(1, 1) == 16 and lib.codon_undistort_tiles_bytes(40, 100) == 5 * 4 * 16
    assert lib.codon_undistort_tiles_bytes(1080, 1920) == 135 * 60 * 16 and lib.codon_undistort_tiles_bytes(4096, 4096) == 512 * 128 * 16
    assert lib.codon_undistort_tiles_bytes(0, 7) == 0 and lib.codon_undistort_tiles_bytes(5, 4097) == 0
    kinds = np.zeros(3, dtype=np.int64)
    for shape in U.SHAPES:
        for rig in U.RIGS:
            M, tiles, counts = U.tables(shape, rig)
            st, msg, got, n = _plan(lib, shape[1], shape[2], M)
            assert st == 0, msg
            assert np.array_equal(got, tiles) and np.array_equal(n, counts), (shape, rig, n.tolist(), counts.tolist())
            assert n[:3].sum() == tiles.shape[0] * tiles.shape[1] and n[3] == (M[..., 0] == U.OUTSIDE).sum()
            kinds += n[:3].astype(np.int64)
            src, dst = U.cameras(shape, rig)
            t2, n2 = D.tile_table(_camera(src), M)
            assert np.array_equal(t2, tiles) and np.array_equal(n2, counts)
    assert (kinds > 0).all()
    # the zoom-out rig on 40 x 100 puts the three kinds into one call
    assert U.tables(U.SHAPES[6], "zoom_out")[2].tolist()[:3] == [10, 3, 7]


def test_plan_refusals():
    lib = L.load()
    shape = U.SHAPES[5]
    M = U.tables(shape, "barrel")[0]
    for at, pair, where in (((3, 5), (32 * 100 - 16, 0), "(3, 5) is (3184, 0)"), ((0, 0), (-17, 0), "(0, 0) is (-17, 0)"),
                            ((39, 99), (0, 32 * 40 - 16), "(39, 99) is (0, 1264)"), ((7, 31), (5, -17), "(7, 31) is (5, -17)"),
                            ((8, 32), (U.OUTSIDE, 0), "(8, 32) is (-1048576, 0)"), ((1, 1), (0, U.OUTSIDE), "(1, 1) is (0, -1048576)")):
        bad = M.copy()
        bad[at] = pair
        st, msg, _, _ = _plan(lib, 40, 100, bad)
        assert st == -1 and msg.startswith("undistort_plan: map entry") and where in msg, msg
        with pytest.raises(RuntimeError, match="undistort_plan failed with status -1: undistort_plan: map entry"):
            D.tile_table(P.Camera(100, 40, 60.0, 60.0, 49.5, 19.5), bad)
    edge = M.copy()
    edge[3, 5] = (32 * 100 - 17, 32 * 40 - 17)                            # the last position inside is accepted
    edge[0, 0] = (-16, -16)
    assert _plan(lib, 40, 100, edge)[0] == 0
    tiles, counts = np.zeros(80, dtype=np.int32), np.zeros(4, dtype=np.uint32)
    m, t, c = P_(M.ctypes.data), P_(tiles.ctypes.data), P_(counts.ctypes.data)
    for args, word in (((40, 100, 40, 100, None, t, c), "null pointer"), ((40, 100, 40, 100, m, None, c), "null pointer"),
                       ((40, 100, 40, 100, m, t, None), "null pointer"), ((0, 100, 40, 100, m, t, c), "a 0x100 source"),
                       ((40, 4097, 40, 100, m, t, c), "a 40x4097 source"), ((40, 100, 0, 100, m, t, c), "a 0x100 target"),
                       ((40, 100, 40, 4097, m, t, c), "a 40x4097 target")):
        assert lib.codon_undistort_plan(*args) == -1
        msg = lib.codon_last_error_string().decode()
        assert msg.startswith("undistort_plan: ") and word in msg, msg


# ---- the refusals of the C entry: on the host, before any HIP call ------------------------------------------------------------------

REFUSALS = (({"src": None}, "null pointer"), ({"map_": None}, "null pointer"), ({"tiles": None}, "null pointer"),
            ({"weights": None}, "null pointer"), ({"out": None}, "null pointer"), ({"B": 0}, "batch 0"), ({"B": 65536}, "batch 65536"),
            ({"hs": 0}, "a 0x7 source"), ({"ws": 4097}, "a 5x4097 source"), ({"ho": 0}, "a 0x7 target"), ({"wo": 4097}, "a 5x4097 target"),
            ({"ch": 0}, "channels 0"), ({"ch": 2}, "channels 2"), ({"ch": 4}, "channels 4"), ({"out": "src"}, "same buffer"),
            ({"map_": "+4"}, "unaligned table"), ({"tiles": "+8"}, "unaligned table"), ({"weights": "+1"}, "unaligned table"))


def undistort_caller(lib, src, map_, tiles, weights, out, stream=None):
    """The good call of REFUSALS -- one grey 5 x 7 image onto 5 x 7 -- over the given addresses, with what a refusal changes as
    keyword arguments ("+n": the good address plus n bytes); shared with the GPU test"""
    good = dict(src=src, map_=map_, tiles=tiles, weights=weights, out=out)

    def call(B=1, hs=5, ws=7, ch=1, ho=5, wo=7, **ptr):
        a = dict(good)
        for k, v in ptr.items():
            a[k] = good[k] + int(v) if isinstance(v, str) and v.startswith("+") else good["src"] if v == "src" else v
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_undistort(B, hs, ws, ch, p(a["src"]), ho, wo, p(a["map_"]), p(a["tiles"]), p(a["weights"]), p(a["out"]), stream)
        return st, lib.codon_last_error_string().decode()
    return call


def undistort_refusals(lib, call):
    for kw, word in REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("undistort: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="undistort failed with status -1: undistort: "):
            L.check(st, "undistort")


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    assert lib.codon_abi_version() == 1
    undistort_refusals(lib, undistort_caller(lib, 4096, 8192, 12288, 16384, 20480))   # never dereferenced: every call is refused


# ---- the module and the command line -----------------------------------------------------------------------------------------------------

def test_module_refusals():
    cam = _camera(U.cameras(U.SHAPES[1], "barrel")[0])
    und = D.Undistortion(cam, device="cpu")                               # the tables are the host's; no call goes through
    assert und.dst == D.out_camera(cam) and set(und.counts) == {"staged", "direct", "empty", "outside"}
    assert und.counts == dict(zip(U.COUNTS, U.tables(U.SHAPES[1], "barrel")[2].tolist()))
    img = torch.zeros((7, 9, 3), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="undistort expects a uint8 tensor, got torch.float32"):
        und(img.float(), 3)
    with pytest.raises(ValueError, match=r"undistort: a tensor of shape \(1, 7, 9, 3\) with channels=1"):
        und(img[None], 1)
    with pytest.raises(ValueError, match=r"undistort: a tensor of shape \(7, 9\) with channels=3"):
        und(img[..., 0], 3)
    with pytest.raises(ValueError, match=r"with channels=3 .*the last dimension is the colour"):
        und(torch.zeros((3, 7, 9), dtype=torch.uint8), 3)
    with pytest.raises(ValueError, match="undistort: a 7x8 image, and the camera is 7x9"):
        und(img[:, :8], 3)
    with pytest.raises(ValueError, match="undistort: a 9x7 image, and the camera is 7x9"):
        und(torch.zeros((2, 9, 7), dtype=torch.uint8))
    with pytest.raises(ValueError, match="undistort: channels 2"):
        und(img, 2)
    with pytest.raises(RuntimeError, match="tensors must live on a HIP device"):
        und(img, 3)
    with pytest.raises(ValueError, match="Undistortion: src must be a Camera"):
        D.Undistortion({"width": 9})


def _rig(dist=(-0.3, 0.1, 1e-3, 1e-3, 0.0)):
    cam = dict(width=9, height=7, fx=5.4, fy=5.6, cx=4.37, cy=2.81)
    return {"depth": dict(cam, dist=[0.1, 0.0, 0.0, 0.0, 0.0]), "color": dict(cam, dist=list(dist)),
            "rotation": [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]], "translation": [0.05, 0.0, 0.0], "note": {"serial": "A17"}}


def test_the_rectified_calibration_is_what_register_accepts():
    m = _rig()
    with pytest.raises(ValueError, match=r"undistort the colour images first \(python -m codon_amd.undistort --calib-out"):
        P.Calibration.from_mapping(m)
    dst = D.out_camera(P.Camera.from_mapping(m["color"], "color"), 0.8)
    r = D.rectified(m, dst)
    cal = P.Calibration.from_mapping(json.loads(json.dumps(r)))
    assert cal.color == dst and cal.color.dist == (0.0,) * 5 and cal.color.fx == 5.4 * 0.8
    assert cal.depth == P.Camera.from_mapping(m["depth"])
    assert {k: v for k, v in r.items() if k != "color"} == {k: v for k, v in m.items() if k != "color"}
    assert m["color"]["dist"] == [-0.3, 0.1, 1e-3, 1e-3, 0.0]             # the argument is untouched
    with pytest.raises(ValueError, match="rectified: dst must be a Camera without distortion"):
        D.rectified(m, P.Camera.from_mapping(m["color"]))
    with pytest.raises(ValueError, match="rectified: the calibration must be a mapping"):
        D.rectified([], dst)


NEEDED = ["--color", "c", "--calib", "c.json", "--out", "o"]


@pytest.mark.parametrize("argv, word", [
    (NEEDED[2:], "--color"), (NEEDED[:2] + NEEDED[4:], "--calib"), (NEEDED[:4], "--out"),
    (NEEDED[:4] + ["--out", "c"], "--out is --color"), (NEEDED[:4] + ["--out", "./x/../c/"], "--out is --color"),
    (NEEDED + ["--focal-scale", "0"], "--focal-scale 0.0 must be positive and finite"),
    (NEEDED + ["--focal-scale", "-1"], "must be positive and finite"), (NEEDED + ["--focal-scale", "nan"], "must be positive and finite"),
    (NEEDED + ["--focal-scale", "inf"], "must be positive and finite"), (NEEDED + ["--focal-scale", "x"], "--focal-scale"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        D.parse_args(argv)
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_command_line_defaults_and_bad_files(tmp_path, capsys):
    a, _ = D.parse_args(NEEDED)
    assert (a.focal_scale, a.gray, a.stats, a.calib_out) == (1.0, False, False, None)
    color = tmp_path / "color"
    color.mkdir()
    rig = tmp_path / "rig.json"
    argv = ["--color", str(color), "--calib", str(rig), "--out", str(tmp_path / "out")]
    for text, word in (("{", "rig.json"), ("[]", "missing color"), (json.dumps({"depth": {}}), "missing color"),
                       (json.dumps({"color": {"width": 9}}), "color lacks height, fx, fy, cx, cy"),
                       (json.dumps({"color": dict(_rig()["color"], dist=[0.1])}), "five numbers")):
        rig.write_text(text)
        with pytest.raises(SystemExit) as e:
            D.main(argv)
        assert e.value.code == 2 and word in capsys.readouterr().err, text
    with pytest.raises(SystemExit) as e:
        D.main(["--color", str(color), "--calib", str(tmp_path / "none.json"), "--out", str(tmp_path / "out")])
    assert e.value.code == 2 and "none.json" in capsys.readouterr().err
    rig.write_text(json.dumps(_rig()))                                    # a calibration register refuses is read here: only color
    with pytest.raises(SystemExit) as e:
        D.main(["--color", str(tmp_path / "nowhere"), "--calib", str(rig), "--out", str(tmp_path / "out")])
    assert e.value.code == 2 and "is not a directory" in capsys.readouterr().err
    if not torch.cuda.is_available():
        with pytest.raises(SystemExit, match="No GPU found"):
            D.main(argv)
        assert not os.path.exists(tmp_path / "out")
