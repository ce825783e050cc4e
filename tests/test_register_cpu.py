"""The depth registration's definition (tests/register_ref.py) on the CPU: what the definition promises -- identity,
exact shifts, the z-test of an occlusion scene, no cracks where a two-corner box leaves them -- its bounds, the host tables of
codon_amd.register against the restatement's, and every refusal that needs no GPU: of the host functions, of the C entry (validated
on the host before any HIP call), of Calibration and of the command line.  Expectations are spelled out here, not derived from the
code under test."""
import ctypes as C
import dataclasses
import json
import re

import numpy as np
import pytest

from codon_amd import _lib as L
from codon_amd import register as P
from tests import register_ref as G

FORMATS = ((np.uint8, 255), (np.uint16, 65535), (np.uint16, 10000))
DYADIC = dict(fx=64.0, fy=32.0, cx=15.5, cy=11.5)
NON_DYADIC = dict(fx=57.3, fy=61.9, cx=15.37, cy=11.81)
EYE = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]


def _cam(h, w, k, dist=(0.0,) * 5, **over):
    return P.Camera(**{**dict(width=w, height=h, dist=dist), **k, **over})


def _tables(cal, scale=1, unit=0.001, radial=False):
    return P.ray_table(cal, radial), P.translation_q20(cal, unit), P.projection_q8(cal, scale)


def _holey(h, w, top, dtype, seed):
    g = np.random.default_rng(seed)
    c = g.integers(1, top + 1, size=(h, w))
    c[g.random((h, w)) < 0.2] = 0
    return c.astype(dtype)


def test_the_host_tables_are_the_restatement():
    """ray_table, translation_q20 and projection_q8 of codon_amd.register give the restatement's bits on every rig of the shared
    cases, distortion and rotation included"""
    for shape in G.SHAPES:
        for calib in G.CALIBS:
            cal = P.Calibration.from_mapping(G.calibration(shape, calib))
            for top in (255, 10000):
                A, T, Q = G.tables(shape, calib, top)
                got = _tables(cal, shape[5], G.unit_of(top))
                assert got[0].dtype == np.int32 and got[1].dtype == np.int64 and got[2].dtype == np.int32
                assert np.array_equal(got[0], A) and np.array_equal(got[1], T) and np.array_equal(got[2], Q), (shape, calib, top)
                assert (cal.color.height // shape[5], cal.color.width // shape[5]) == shape[3:5]
    d = G.calibration(G.SHAPES[3], "mixed")["depth"]
    rad = G.ray_table(17, 33, d["fx"], d["fy"], d["cx"], d["cy"], d["dist"], G.calibration(G.SHAPES[3], "mixed")["rotation"], radial=True)
    assert np.array_equal(P.ray_table(P.Calibration.from_mapping(G.calibration(G.SHAPES[3], "mixed")), radial=True), rad)


@pytest.mark.parametrize("k", [DYADIC, NON_DYADIC], ids=["dyadic", "non_dyadic"])
@pytest.mark.parametrize("dtype, top", FORMATS, ids=["u8", "u16", "u16_10000"])
def test_identity_returns_the_plane(k, dtype, top):
    """One camera in both roles, no motion, scale 1: the plane comes back bit for bit, holes included"""
    h, w = 24, 32
    cal = P.Calibration(_cam(h, w, k), _cam(h, w, k), EYE, (0.0, 0.0, 0.0))
    c = _holey(h, w, top, dtype, 7)
    out, stats = G.register_plane(c, *_tables(cal), h, w, top)
    assert out.dtype == c.dtype and np.array_equal(out, c)
    valid = int((c != 0).sum())
    assert stats.tolist() == [valid, 0, 0, valid]


@pytest.mark.parametrize("k", [DYADIC, NON_DYADIC], ids=["dyadic", "non_dyadic"])
@pytest.mark.parametrize("dx, dy", [(3, 0), (0, -2), (-5, 4)])
def test_a_principal_point_shift_is_an_exact_shift(k, dx, dy):
    """The colour principal point moved by (dx, dy) whole pixels: out[y + dy, x + dx] = in[y, x], and the valid pixels of the rows
    and columns that leave the image are the `outside` count"""
    h, w, top = 24, 32, 10000
    cal = P.Calibration(_cam(h, w, k), _cam(h, w, k, cx=k["cx"] + dx, cy=k["cy"] + dy), EYE, (0.0, 0.0, 0.0))
    c = _holey(h, w, top, np.uint16, 11)
    out, stats = G.register_plane(c, *_tables(cal), h, w, top)
    want = np.zeros_like(c)
    ys, xs = np.arange(h), np.arange(w)
    ky, kx = (ys + dy >= 0) & (ys + dy < h), (xs + dx >= 0) & (xs + dx < w)
    want[np.ix_(ys[ky] + dy, xs[kx] + dx)] = c[np.ix_(ys[ky], xs[kx])]
    assert np.array_equal(out, want)
    stay = int((c[np.ix_(ys[ky], xs[kx])] != 0).sum())
    valid = int((c != 0).sum())
    assert stats.tolist() == [valid, valid - stay, 0, stay]


def test_the_occlusion_scene():
    """A background at 3000 codes, an 8 x 8 foreground square at 1000, the colour camera 200 codes to the side: the square moves
    fx 200 / 1000 = 12 columns, the background fx 200 / 3000 = 4; where both land the square wins, and what it uncovered is a hole"""
    h, w, top, fx = 32, 64, 65535, 60.0
    k = dict(fx=fx, fy=fx, cx=31.5, cy=15.5)
    cal = P.Calibration(_cam(h, w, k), _cam(h, w, k), EYE, (0.2, 0.0, 0.0))          # 200 codes of 1 mm
    assert P.translation_q20(cal, 0.001).tolist() == [200 << 20, 0, 0]
    c = np.full((h, w), 3000, dtype=np.uint16)
    c[12:20, 20:28] = 1000
    out, stats = G.register_plane(c, *_tables(cal), h, w, top)
    assert set(np.unique(out)) == {0, 1000, 3000}
    want = np.zeros_like(c)
    want[:, 4:] = 3000                              # the background, four columns on; its last four columns left the image
    want[12:20, 24:32] = 0                          # where the square stood, seen from the side: nothing was measured
    want[12:20, 32:40] = 1000                       # the square, twelve columns on, in front of the background that lands there too
    assert np.array_equal(out, want)
    assert stats.tolist() == [h * w, 4 * h, 0, int((want != 0).sum())]
    # the other way round the square hides part of the background and the hole opens on its other side
    back = P.Calibration(_cam(h, w, k), _cam(h, w, k), EYE, (-0.2, 0.0, 0.0))
    out2, _ = G.register_plane(c, *_tables(back), h, w, top)
    want2 = np.zeros_like(c)
    want2[:, :60] = 3000
    want2[12:20, 16:24] = 0
    want2[12:20, 8:16] = 1000
    assert np.array_equal(out2, want2)


# ---- no cracks ------------------------------------------------------------------------------------------------------------------------

GRIDS = {"finer": (60, 80), "equal": (24, 32), "coarser": (12, 16)}
ROTATIONS = {"roll_0.1": (0.0, 0.0, 0.1), "roll_0.4": (0.0, 0.0, 0.4), "mixed": (0.05, -0.08, 0.2)}


def _crack_case(grid, rot, slanted):
    hs, ws, top = 24, 32, 10000
    ho, wo = GRIDS[grid]
    fd = 40.0
    depth = P.Camera(ws, hs, fd, fd, (ws - 1) / 2, (hs - 1) / 2)
    fc = fd * wo / ws
    color = P.Camera(wo, ho, fc, fc, (wo - 1) / 2, (ho - 1) / 2)
    cal = P.Calibration(depth, color, G.rotation(*ROTATIONS[rot]).tolist(), (0.03, -0.02, 0.01))
    j, i = np.meshgrid(np.arange(ws), np.arange(hs))
    c = (2000 + (25 * j + 10 * i if slanted else 0 * j)).astype(np.uint16)
    return c, _tables(cal), ho, wo, top


@pytest.mark.parametrize("slanted", [False, True], ids=["flat", "slanted"])
@pytest.mark.parametrize("rot", list(ROTATIONS))
@pytest.mark.parametrize("grid", list(GRIDS))
def test_no_cracks(grid, rot, slanted):
    """A plane seen by a rolled, turned and shifted camera, onto a grid 2.5 x finer, equal and 2 x coarser: the four-corner box
    leaves no hole with filled neighbours on both sides; the box of the diagonal's two corners -- written here -- does, so the
    property bites."""
    c, (A, T, Q), ho, wo, top = _crack_case(grid, rot, slanted)
    U, V, z, valid, kept = G.project(c, A, T, Q, top)
    assert kept.all()
    out, stats, over = G.splat(U, V, z, valid, kept, ho, wo)
    assert over == 0 and stats[2] == 0 and stats[3] > ho * wo // 4
    assert G.cracks(out) == 0
    two, _, _ = G.splat(U[:2], V[:2], z, valid, kept, ho, wo)          # the corners a and b alone
    print(f"{grid} {rot} {'slanted' if slanted else 'flat'}: two-corner cracks {G.cracks(two)}, filled {int(stats[3])} of {ho * wo}")
    assert G.cracks(two) > 0
    assert ((two != 0) <= (out != 0)).all()                            # the two-corner box is a part of the four-corner box


# ---- the bounds -------------------------------------------------------------------------------------------------------------------------

def test_the_intermediates_at_the_bounds_fit_64_bits():
    """Python ints: at |A| = 2^22 - 1, |T| = 2^38 - 1, k = 65535, FX = 2^20 - 1, |CX| = 2^21 - 1 every intermediate is below 2^61,
    hence below 2^63, and a quotient below 2^41"""
    a, t, k, fx, cx = G.A_LIMIT - 1, G.T_LIMIT - 1, 65535, G.F_LIMIT - 1, G.C_LIMIT - 1
    assert (a, t, fx, cx) == (2 ** 22 - 1, 2 ** 38 - 1, 2 ** 20 - 1, 2 ** 21 - 1)
    p = k * a + t                                   # the largest |P| component
    assert k * a < 2 ** 38 and p < 2 ** 39
    num = fx * p + cx * p                           # |FX P.x + CX P.z| at its largest
    assert fx * p < 2 ** 59 and cx * p < 2 ** 60 and num < 2 ** 61 < 2 ** 63
    assert (p + p + 1) // 2 + 2 ** 19 < 2 ** 40     # z' before its shift
    q = fx * p // G.ONE + cx                        # the largest |U|: P.z at its smallest, 2^20
    assert q < 2 ** 41 and q + 255 < 2 ** 63
    assert num + p < 2 ** 62                        # an estimate of the quotient one off, times its denominator
    # and the restatement runs there without wrapping: one pixel, every table at its bound
    A = np.full((2, 2, 3), a, dtype=np.int32)
    U, V, z, valid, kept = G.project(np.array([[k]], dtype=np.uint16), A, [t, t, t], [fx, fx, cx, cx], 65535)
    assert valid.all() and not kept.any()           # z' = (k a + t + 2^19) >> 20 lies far above top: dropped
    A[..., 2] = G.ONE
    U, V, z, valid, kept = G.project(np.array([[k]], dtype=np.uint16), A, [t, t, 0], [fx, fx, cx, cx], 65535)
    assert kept.all() and int(z[0, 0]) == k and int(U[0, 0, 0]) == (fx * (k * a + t) + cx * k * G.ONE) // (k * G.ONE)


def test_one_past_each_bound_is_refused_by_name():
    ok = dict(fx=60.0, fy=60.0, cx=15.5, cy=11.5)
    cal = lambda depth=None, color=None, t=(0.0, 0.0, 0.0): P.Calibration(                                    # noqa: E731
        depth or _cam(24, 32, ok), color or _cam(24, 32, ok), EYE, t)
    # |A| >= 2^22: a corner with |x_n| >= 4
    with pytest.raises(ValueError, match="ray_table: a corner ray of 2\\^22 or more"):
        P.ray_table(cal(depth=_cam(24, 32, ok, fx=4.0)))                     # x_n = (32 - 0.5 - 15.5) / 4 = 4
    assert np.abs(P.ray_table(cal(depth=_cam(24, 32, ok, fx=4.0001)))).max() == G.A_LIMIT - 105
    # |T| >= 2^38: 2^18 codes
    assert P.translation_q20(cal(t=(262143.999, 0, 0)), 1.0)[0] == G.T_LIMIT - 1049
    for t in ((262144.0, 0, 0), (0, -262144.0, 0), (0, 0, 262.144)):
        with pytest.raises(ValueError, match="translation_q20: a translation of"):
            P.translation_q20(cal(t=t), 1.0 if t[2] == 0 else 0.001)
    for unit in (0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="translation_q20: depth_unit"):
            P.translation_q20(cal(), unit)
    # FX, FY >= 2^20: 4096 pixels at scale 1
    assert P.projection_q8(cal(color=_cam(24, 32, ok, fx=4095.998)), 1)[0] == G.F_LIMIT - 1
    with pytest.raises(ValueError, match="projection_q8: focal lengths"):
        P.projection_q8(cal(color=_cam(24, 32, ok, fx=4096.0)), 1)
    with pytest.raises(ValueError, match="projection_q8: focal lengths"):
        P.projection_q8(cal(color=_cam(24, 32, ok, fy=4096.0)), 1)
    assert P.projection_q8(cal(color=_cam(24, 32, ok, fx=4096.0 * 16 - 1)), 16)[0] == G.F_LIMIT - 16
    with pytest.raises(ValueError, match="projection_q8: focal lengths"):
        P.projection_q8(cal(color=_cam(24, 32, ok, fx=0.001)), 16)           # FX = 0
    # |CX|, |CY| >= 2^21: 8192 pixels at scale 1
    assert P.projection_q8(cal(color=_cam(24, 32, ok, cx=8191.996)), 1)[2] == G.C_LIMIT - 1
    with pytest.raises(ValueError, match="projection_q8: principal point"):
        P.projection_q8(cal(color=_cam(24, 32, ok, cx=8192.0)), 1)
    with pytest.raises(ValueError, match="projection_q8: principal point"):
        P.projection_q8(cal(color=_cam(24, 32, ok, cy=-8192.0)), 1)
    with pytest.raises(ValueError, match="projection_q8: scale 2 "):
        P.projection_q8(cal(), 2)


# ---- the refusals of the C entry: on the host, before any HIP call ------------------------------------------------------------------

def register_refusals(lib, call):
    """call(**what differs) -> (status, message) of codon_register_depth; shared with the GPU test"""
    for kw, word in G.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("register_depth: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="register_depth failed with status -1: register_depth: "):
            L.check(st, "register_depth")


def register_caller(lib, src, rays, out, ws, stats=None, stream=None):
    """The good call of register_ref.REFUSALS -- u16 codes, a 5 x 7 source onto 3 x 5 -- over the given addresses, with what a
    refusal changes as keyword arguments"""
    P_ = C.c_void_p

    def call(B=1, hs=5, ws_=7, src=src, fmt=L.FILL_U16, top=65535, rays=rays, T=(1 << 20, 0, 0), P=(256, 256, 0, 0), trans=True,
             proj=True, ho=3, wo=5, out=out, stats=stats, ws=ws, ws_bytes=None):
        need = B * lib.codon_register_workspace_bytes(ho, wo) if B > 0 else 0
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_register_depth(B, hs, ws_, p(src), fmt, top, p(rays), (C.c_int64 * 3)(*T) if trans else None,
                                      (C.c_int32 * 4)(*P) if proj else None, ho, wo, p(out), p(stats), p(ws), ws_bytes, stream)
        return st, lib.codon_last_error_string().decode()
    return call


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    assert lib.codon_register_workspace_bytes(3, 5) == 64 and lib.codon_register_workspace_bytes(270, 480) == 270 * 480 * 4
    assert lib.codon_register_workspace_bytes(0, 7) == 0 and lib.codon_register_workspace_bytes(5, 4097) == 0
    assert lib.codon_abi_version() == 1
    call = register_caller(lib, 4096, 8192, 12288, 16384)           # never dereferenced: every call is refused on the host
    register_refusals(lib, call)
    for kw in ({"src": 4097}, {"out": 12289}, {"rays": 8194}, {"stats": 20482}, {"ws": 16392}):
        assert "unaligned" in call(**kw)[1], kw
    # at the bounds themselves the refusal is the short workspace asked for beside them: no bound is off by one
    at = dict(T=(G.T_LIMIT - 1, 1 - G.T_LIMIT, 0), P=(G.F_LIMIT - 1, 1, G.C_LIMIT - 1, 1 - G.C_LIMIT), ws_bytes="short")
    assert "too small" in call(**at)[1]


# ---- the tables -------------------------------------------------------------------------------------------------------------------------

def test_undistortion_returns_the_corner():
    """The undistorted corner, distorted again by the Brown model, is the corner to 1e-9 pixels (the float64 rays ray_table rounds)"""
    dist = (-0.3, 0.1, 1e-3, 1e-3, 0.0)
    cam = P.Camera(64, 48, 60.0, 61.0, 31.2, 23.7, dist)
    r = P.corner_rays(cam)
    assert r.shape == (49, 65, 3) and (r[..., 2] == 1.0).all()
    k1, k2, p1, p2, k3 = dist                                           # the Brown model, spelled out
    x, y = r[..., 0], r[..., 1]
    r2 = x * x + y * y
    rad = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
    xd = x * rad + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rad + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    j, i = np.meshgrid(np.arange(65.0), np.arange(49.0))
    err = max(np.abs(xd * cam.fx + cam.cx - (j - 0.5)).max(), np.abs(yd * cam.fy + cam.cy - (i - 0.5)).max())
    print(f"undistortion: {err:.3g} pixels; the corner moved by up to {np.abs(x * cam.fx + cam.cx - (j - 0.5)).max():.2f}")
    assert err <= 1e-9
    assert np.abs(x * cam.fx + cam.cx - (j - 0.5)).max() > 1.0          # and the distortion is no nothing
    plain = P.corner_rays(P.Camera(64, 48, 60.0, 61.0, 31.2, 23.7))
    assert np.array_equal(plain[..., 0], (j - 0.5 - 31.2) / 60.0)


def test_ranges_along_the_ray_give_the_wall():
    """A fronto-parallel wall at z = 3000 codes: the file of ranges, registered with radial=True, equals the file of z registered
    with radial=False to +-1 code"""
    h, w, top, Z = 48, 64, 10000, 3000
    k = dict(fx=200.0, fy=200.0, cx=31.5, cy=23.5)
    cal = P.Calibration(_cam(h, w, k), _cam(h, w, k), EYE, (0.0, 0.0, 0.0))
    j, i = np.meshgrid(np.arange(w), np.arange(h))
    ranges = np.rint(Z * np.sqrt(((j - 31.5) / 200.0) ** 2 + ((i - 23.5) / 200.0) ** 2 + 1.0)).astype(np.uint16)
    assert ranges.max() > Z + 30
    a, _ = G.register_plane(np.full((h, w), Z, dtype=np.uint16), *_tables(cal), h, w, top)
    b, _ = G.register_plane(ranges, *_tables(cal, radial=True), h, w, top)
    assert (a == Z).all() and (b != 0).all()
    assert np.abs(b.astype(np.int64) - a.astype(np.int64)).max() <= 1


# ---- Calibration and the command line ---------------------------------------------------------------------------------------------------

def _mapping(**over):
    m = json.loads(json.dumps(G.calibration(G.SHAPES[3], "mixed")))
    m.update(over)
    return m


def test_calibration_reads_a_mapping_and_a_file(tmp_path):
    m = _mapping()
    cal = P.Calibration.from_mapping(m)
    assert cal.depth.dist == tuple(G.DIST_MIXED) and cal.color.dist == (0.0,) * 5 and cal.translation == tuple(G.T_MIXED)
    assert np.array_equal(np.array(cal.rotation), np.array(m["rotation"]))
    path = tmp_path / "rig.json"
    path.write_text(json.dumps(m))
    assert P.Calibration.from_json(str(path)) == cal
    with pytest.raises(dataclasses.FrozenInstanceError):
        cal.translation = (0, 0, 0)
    del m["depth"]["dist"]                                               # dist may be left out: no distortion
    assert P.Calibration.from_mapping(m).depth.dist == (0.0,) * 5


def _drop(cam, key):
    m = _mapping()
    del m[cam][key]
    return m


@pytest.mark.parametrize("m, word", [
    (_mapping(rotation=[[1, 0, 0], [0, 1, 0], [0, 0, 1.001]]), "rotation is not orthonormal"),
    (_mapping(rotation=[[2, 0, 0], [0, 2, 0], [0, 0, 2]]), "rotation is not orthonormal"),
    (_mapping(rotation=[[1, 0, 0], [0, 1, 0]]), "rotation must be 3 x 3"),
    (_mapping(rotation=[[1, 0, 0], [0, float("nan"), 0], [0, 0, 1]]), "rotation .* is not finite"),
    (_mapping(translation=[0, 0]), "translation must be three numbers"),
    (_mapping(translation=[0, float("inf"), 0]), "translation .* is not finite"),
    (_mapping(color=dict(_mapping()["color"], dist=[0, 0, 1e-3, 0, 0])), "undistort the colour images first"),
    ({k: v for k, v in _mapping().items() if k != "rotation"}, "Calibration: missing rotation"),
    ({k: v for k, v in _mapping().items() if k not in ("depth", "translation")}, "Calibration: missing depth, translation"),
    (_drop("depth", "fx"), "Calibration: depth lacks fx"),
    (_drop("color", "height"), "Calibration: color lacks height"),
    (_mapping(depth=dict(_mapping()["depth"], fx=float("nan"))), "fx, fy, cx, cy .* is not finite"),
    (_mapping(depth=dict(_mapping()["depth"], fy=0.0)), "focal lengths .* must be positive"),
    (_mapping(depth=dict(_mapping()["depth"], dist=[0, 0, 0])), "dist .* \\(five numbers"),
    (_mapping(depth=dict(_mapping()["depth"], dist=[0, 0, 0, 0, float("inf")])), "dist .* is not finite"),
    (_mapping(depth=dict(_mapping()["depth"], width=0)), "width 0 "),
    (_mapping(color=dict(_mapping()["color"], height=4097)), "height 4097 "),
    (_mapping(color=dict(_mapping()["color"], width=80.5)), "width 80.5 "),
    ([1, 2], "the calibration must be a mapping"),
])
def test_calibration_refusals(m, word):
    with pytest.raises(ValueError, match=word):
        P.Calibration.from_mapping(m)


def test_calibration_file_refusals(tmp_path):
    bad = tmp_path / "bad.json"
    bad.write_text("{not json")
    with pytest.raises(ValueError, match="Calibration: .*bad.json"):
        P.Calibration.from_json(str(bad))
    with pytest.raises(OSError):
        P.Calibration.from_json(str(tmp_path / "none.json"))


NEEDED = ["--depth", "d", "--calib", "c.json", "--out", "o"]


@pytest.mark.parametrize("argv, word", [
    (["--calib", "c.json", "--out", "o"], "the following arguments are required: --depth"),
    (["--depth", "d", "--out", "o"], "the following arguments are required: --calib"),
    (["--depth", "d", "--calib", "c.json"], "the following arguments are required: --out"),
    ([*NEEDED, "--scale", "2"], "invalid choice"),
    ([*NEEDED, "--depth-bits", "12"], "invalid choice"),
    ([*NEEDED, "--depth-max", "10000"], "--depth-max needs --depth-bits 16"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "0"], "--depth-max 0 must be in \\[1, 65535\\]"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "65536"], "--depth-max 65536 must be in"),
    ([*NEEDED, "--depth-unit", "0"], "--depth-unit 0.0 must be positive"),
    ([*NEEDED, "--depth-unit", "-0.001"], "--depth-unit -0.001 must be positive"),
    ([*NEEDED, "--depth-unit", "nan"], "--depth-unit nan must be positive"),
    (["--depth", "d", "--calib", "c.json", "--out", "./d"], "--out is --depth"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        P.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_command_line_defaults_and_a_bad_calibration_file(tmp_path, capsys):
    a, _ = P.parse_args(NEEDED)
    assert (a.scale, a.depth_bits, a.depth_max, a.depth_unit, a.radial, a.stats) == (1, 8, None, 0.001, False, False)
    a, _ = P.parse_args([*NEEDED, "--scale", "4", "--depth-bits", "16", "--depth-max", "10000", "--depth-unit", "0.00025", "--radial",
                         "--stats"])
    assert (a.scale, a.depth_bits, a.depth_max, a.depth_unit, a.radial, a.stats) == (4, 16, 10000, 0.00025, True, True)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(_mapping(translation=[0, 0])))
    with pytest.raises(SystemExit) as e:                                 # the calibration is read before the GPU is asked for
        P.main(["--depth", str(tmp_path), "--calib", str(rig), "--out", str(tmp_path / "o")])
    assert e.value.code == 2 and "translation must be three numbers" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        P.main(["--depth", str(tmp_path), "--calib", str(tmp_path / "none.json"), "--out", str(tmp_path / "o")])
    assert e.value.code == 2 and "none.json" in capsys.readouterr().err
