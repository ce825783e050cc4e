"""The point clouds with normals without a GPU: the numpy restatement tests/cloud_ref.py against what the definition
promises -- its bounds in Python integers at their extremes, planes whose normals are known, edges, holes, mirrors -- and the
host functions of codon_amd.cloud: the ray tables, the PLY header, writer and reader, and every refusal of Unprojection, of the
C entries (refused on the host, before any HIP call) and of the command line."""
import ctypes as C
import json
import math
import re

import numpy as np
import pytest

from codon_amd import _lib as L
from codon_amd import cloud as K
from codon_amd import register as P
from tests import cloud_ref as R

RQ = R.rel_q16(0.02)
CAM = dict(width=60, height=40, fx=500.0, fy=500.0, cx=29.5, cy=19.5)


def _normals(c, rx, ry, radius=2, A=2, Rq=RQ):
    return R.normals_q14(c, rx, ry, radius, A, Rq)


# ---- the definition ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radius", [1, 2, 8])
def test_constant_plane_faces_the_camera_everywhere(radius):
    """A fronto-parallel plane: exactly (0, 0, -16384) in the interior (two-sided tangents) and at the border (one-sided)"""
    rx, ry = R.ray_tables(23, 19, 31.0, 29.0, 10.25, 8.75)
    for k in (1, 77, 1234, 65535):
        N, has = _normals(np.full((19, 23), k, dtype=np.uint16), rx, ry, radius)
        assert has.all() and (N == np.array([0, 0, -R.ONE])).all(), (radius, k)


def test_every_bound_at_its_extreme():
    """In Python integers: k = 65535, |R| = 2^22 - 1, radius 8"""
    k, ray = 65535, R.RAY_LIMIT - 1
    p = k * ray
    assert p < 1 << 38 and (k << 20) < 1 << 38
    p8 = (p + 2048) >> 12
    assert p8 < (1 << 26) + 1 and abs((-p + 2048) >> 12) < (1 << 26) + 1
    d = 2 * p8                                                        # a tangent component: P8+ - P8- at most
    assert d * d < 1 << 54 and 2 * d * d < 1 << 55                    # a product, a component of the cross product
    assert 8 * 65535 + ((65535 * 65535) >> 16) < 1 << 32              # R A + ((Rq min) >> 16) in unsigned 32 bits
    # the reduction leaves |n_c| < 2^30, so n . n < 3 2^60 and n . P8 < 3 2^56: both fit int64
    for n in (2 * d * d, (1 << 55) - 1, (1 << 30) + 5, (1 << 30) - 1, 12345):
        s = max(0, n.bit_length() - 30)
        assert (n >> s) < 1 << 30 and (s == 0 or (n >> s) >= 1 << 29)
    top = (1 << 30) - 1
    assert 3 * top * top < 3 << 60 < 1 << 63 and 3 * top * p8 < 1 << 63
    # the root: the fp64 estimate, floored, is within one of isqrt at the extremes and around squares
    worst = 0
    for L0 in (1, 2, 3, 1 << 15, (1 << 26) + 1, 94906265, 94906266, 94906267, 1 << 30, 1859775393, int(math.isqrt(3 * top * top))):
        for s in (L0 * L0 - 1, L0 * L0, L0 * L0 + 1, L0 * L0 + L0, (L0 + 1) * (L0 + 1) - 1):
            if 0 <= s <= 3 * top * top:
                worst = max(worst, abs(int(math.sqrt(float(s))) - math.isqrt(s)))
    assert worst <= 1
    # the quotient: |2 n 16384 + L| < 2^46 and 2 L < 2^32 are exact in fp64, the quotient at most 16384 in magnitude
    L0 = math.isqrt(3 * top * top)
    assert 2 * top * R.ONE + L0 < 1 << 46 and 2 * L0 < 1 << 32
    for n in (top, -top, 0, 1, -1):
        L1 = math.isqrt(n * n)
        if L1:
            assert abs((2 * n * R.ONE + L1) // (2 * L1)) <= R.ONE
    assert 128 + ((127 * R.ONE + 8192) >> 14) == 255 and 128 + ((127 * -R.ONE + 8192) >> 14) == 1 and 128 + (8192 >> 14) == 128


def test_normal_map_formula():
    """+-16384 and 0 of a normal, and (0, 0, 0) for a hole and for a pixel without a normal"""
    rx, ry = R.ray_tables(9, 7, 20.0, 20.0, 4.0, 3.0)
    c = np.full((7, 9), 500, dtype=np.uint16)
    c[3, 4] = 0
    c[0, 0] = 60000                                                   # linked to nothing: no normal
    rec, counts, nmap = R.cloud_plane(c, rx, ry)
    assert nmap.dtype == np.uint8 and nmap.shape == (7, 9, 3)
    assert nmap[3, 4].tolist() == [0, 0, 0] and nmap[0, 0].tolist() == [0, 0, 0] and nmap[5, 5].tolist() == [128, 128, 1]
    # without a normal: (0, 0), and (1, 4) and (5, 4), whose far pixels along y are the hole and outside the plane
    assert nmap[1, 4].tolist() == [0, 0, 0] and nmap[5, 4].tolist() == [0, 0, 0]
    assert counts.tolist() == [62, 59] and rec["nz"][0] == 0.0 and rec["nz"][1] == -1.0


def test_positions_reproject_to_their_pixel():
    """x / z fx + cx lies within fx 2^-21 (the table's rounding) plus float32 rounding of j, and y likewise"""
    g = np.random.default_rng(3)
    w, h, fx, fy, cx, cy = 60, 40, 513.7, 498.2, 29.3, 19.9
    rx, ry = R.ray_tables(w, h, fx, fy, cx, cy)
    c = g.integers(1, 65536, size=(h, w)).astype(np.uint16)
    rec, _, _ = R.cloud_plane(c, rx, ry, normals=False)
    i, j = np.divmod(np.arange(h * w), w)
    x, y, z = (rec[n].astype(np.float64) for n in "xyz")
    assert np.array_equal(rec["z"], (c.ravel().astype(np.float64) * 0.001).astype(np.float32))
    # three float32 roundings, each 2^-24 relative, of a ratio at most max(w / fx, h / fy) < 1 in magnitude
    assert np.abs(x / z * fx + cx - j).max() <= fx * 2.0 ** -21 + 3 * fx * 2.0 ** -24
    assert np.abs(y / z * fy + cy - i).max() <= fy * 2.0 ** -21 + 3 * fy * 2.0 ** -24


def test_records_are_the_valid_pixels_in_row_major_order():
    shape = R.SHAPES[5]
    rx, ry = R.tables(shape)
    c = R.plane(shape, "random")[1]
    rgb = R.tint(shape, 3)[1]
    rec, counts, _ = R.cloud_plane(c, rx, ry, color=rgb)
    i, j = np.nonzero(c)                                              # row-major
    assert len(rec) == counts[0] == (c != 0).sum() and rec.dtype.itemsize == 27
    assert np.array_equal(rec["z"], (c[i, j].astype(np.float64) * 0.001).astype(np.float32))
    assert np.array_equal(np.stack([rec["red"], rec["green"], rec["blue"]], axis=1), rgb[i, j])
    grey, _, _ = R.cloud_plane(c, rx, ry, normals=False, color=rgb[..., 0])
    assert grey.dtype.itemsize == 15 and np.array_equal(grey["red"], grey["blue"]) and np.array_equal(grey["green"], rgb[i, j, 0])


@pytest.mark.parametrize("radius", [1, 2, 4])
def test_two_surfaces_never_mix(radius):
    """Every normal within R pixels of the edge equals what its surface alone gives"""
    top, h, w, edge = 10000, 24, 40, 20
    rx, ry = R.ray_tables(w, h, 45.0, 44.0, 19.25, 11.5)
    c = R.two_surfaces(top, h, w, edge)
    N, has = _normals(c, rx, ry, radius, 20)
    near, far = np.full((h, w), c[0, 0]), np.full((h, w), c[0, -1])
    Nn, Nf = _normals(near, rx, ry, radius, 20)[0], _normals(far, rx, ry, radius, 20)[0]
    assert has.all() and np.array_equal(N[:, :edge], Nn[:, :edge]) and np.array_equal(N[:, edge:], Nf[:, edge:])
    assert (N[..., 2] == -R.ONE).all()
    # without the link rule the tangents across the edge would differ: the rule is what the test is about
    loose, _ = _normals(c, rx, ry, radius, 10000)
    assert not np.array_equal(loose[:, edge - radius:edge + radius], N[:, edge - radius:edge + radius])


def test_no_tangent_on_one_axis_no_normal_but_a_point():
    rx, ry = R.ray_tables(9, 9, 20.0, 20.0, 4.0, 4.0)
    c = np.full((9, 9), 800, dtype=np.uint16)
    c[4, 2] = c[4, 6] = 0                                             # both far pixels of (4, 4) along x are holes
    c[1, 1] = 0
    c[2, 7] = 300                                                     # unlinked to everything
    rec, counts, nmap = R.cloud_plane(c, rx, ry)
    N, has = _normals(c, rx, ry)
    assert not has[4, 4] and not has[2, 7] and not has[1, 1] and has[4, 5] and has[3, 1]
    # without a normal: (4, 4); (4, 0) and (4, 8), which look at a hole and outside the plane; (2, 7); (0, 7), which looks at (2, 7)
    assert not has[4, 8] and not has[0, 7] and has[2, 5] and has[4, 7]
    assert counts.tolist() == [78, 73] and len(rec) == 78
    at = int((c != 0).ravel()[:4 * 9 + 4].sum())                      # (4, 4)'s rank
    assert rec["z"][at] == np.float32(0.8) and (rec["nx"][at], rec["ny"][at], rec["nz"][at]) == (0.0, 0.0, 0.0)
    assert not has[4, 0] and has[3, 0]


@pytest.mark.parametrize("h, w", [(1, 1), (1, 9), (9, 1), (2, 2), (2, 9), (3, 3)])
def test_planes_no_larger_than_the_radius(h, w):
    """h or w <= R = 2: no pixel along that axis is inside the plane, so there is no normal; at 3 the ends of an axis see each other"""
    rx, ry = R.ray_tables(w, h, 20.0, 20.0, 0.5, 0.25)
    rec, counts, nmap = R.cloud_plane(np.full((h, w), 900, dtype=np.uint16), rx, ry)
    want = 0 if min(h, w) <= 2 else 4
    assert counts.tolist() == [h * w, want] and int((nmap.reshape(-1, 3).any(axis=1)).sum()) == want
    assert (rec["nz"] != 0).sum() == want


def test_mirror():
    """The image flipped left to right with cx -> w - 1 - cx: x and nx change sign, nothing else changes (and up-down likewise)"""
    w, h, fx, fy, cx, cy = 41, 25, 37.0, 35.0, 18.25, 13.5            # cx, cy exact in binary: the mirrored tables are exact negatives
    c = R.plane((1, h, w), "random", seed=2)[0]                        # a seed without a tie (below)
    rx, ry = R.ray_tables(w, h, fx, fy, cx, cy)
    fxx, _ = R.ray_tables(w, h, fx, fy, w - 1 - cx, cy)
    _, fyy = R.ray_tables(w, h, fx, fy, cx, h - 1 - cy)
    assert np.array_equal(fxx, -rx[::-1]) and np.array_equal(fyy, -ry[::-1])
    P = R.points_q20(c, rx, ry)
    assert not ((P[..., :2] & 4095) == 2048).any()                    # no P8 at a tie: >> 12 rounds -v as -(v rounded)
    N, has = _normals(c, rx, ry, 2, 20)
    Nx, hasx = _normals(c[:, ::-1], fxx, ry, 2, 20)
    Ny, hasy = _normals(c[::-1], rx, fyy, 2, 20)
    assert has.sum() > 300
    assert np.array_equal(hasx[:, ::-1], has) and np.array_equal(Nx[:, ::-1], N * np.array([-1, 1, 1]))
    assert np.array_equal(hasy[::-1], has) and np.array_equal(Ny[::-1], N * np.array([1, -1, 1]))
    assert np.array_equal(R.points_q20(c[:, ::-1], fxx, ry)[:, ::-1], P * np.array([-1, 1, 1]))


def test_int16_view_is_read_as_unsigned():
    shape = R.SHAPES[5]
    rx, ry = R.tables(shape)
    c = R.plane(shape, "high")[0]
    assert (c >= 32768).sum() > 100
    a, ca, ma = R.cloud_plane(c, rx, ry, tolerance=131)
    b, cb, mb = R.cloud_plane(c.view(np.int16), rx, ry, tolerance=131)
    assert a.tobytes() == b.tobytes() and np.array_equal(ca, cb) and np.array_equal(ma, mb) and ca[1] > 0


# the issue's prototype measured the same maxima over the pixels whose tangents are two-sided, R or more from the border
SLANT = {(10000, 2000): {1: 5.49, 2: 2.36, 4: 1.10}, (65535, 20000): {1: 0.42, 2: 0.22, 4: 0.13}}
# over ALL pixels, one-sided tangents at the border included (measured with this restatement)
SLANT_ALL = {(10000, 2000): {1: 5.49, 2: 5.08, 4: 1.87}, (65535, 20000): {1: 0.42, 2: 0.37, 4: 0.20}}


@pytest.mark.parametrize("top, z0", list(SLANT))
@pytest.mark.parametrize("radius", [1, 2, 4])
def test_slanted_plane_against_the_analytic_normal(top, z0, radius):
    """Z = z0 / (1 - 0.5 x_n), 40 x 60, fx = fy = 500: the angle to the ANALYTIC normal; what this restatement measures is the
    table above to its last digit, and the bound is twice that"""
    c, n = R.slanted_plane(top, z0)
    rx, ry = R.ray_tables(CAM["width"], CAM["height"], CAM["fx"], CAM["fy"], CAM["cx"], CAM["cy"])
    N, has = _normals(c, rx, ry, radius, max(2, top // 500))
    assert has.all()
    v = N.astype(np.float64) / R.ONE
    assert np.abs(np.linalg.norm(v, axis=2) - 1.0).max() < 2e-4      # three components rounded to 2^-15 each
    ang = np.degrees(np.arccos(np.clip((v @ n) / np.linalg.norm(v, axis=2), -1.0, 1.0)))
    inner, whole = ang[radius:-radius, radius:-radius].max(), ang.max()
    print(f"top {top} z0 {z0} R {radius}: two-sided {inner:.3f} deg, all pixels {whole:.3f} deg")
    assert round(inner, 2) == SLANT[(top, z0)][radius] and round(whole, 2) == SLANT_ALL[(top, z0)][radius]
    assert inner <= 2 * SLANT[(top, z0)][radius] and whole <= 2 * SLANT_ALL[(top, z0)][radius]


# ---- the host functions ---------------------------------------------------------------------------------------------------------------

def test_ray_tables_equal_the_restatement_and_scale():
    cam = P.Camera(**CAM)
    rx, ry = K.ray_tables(cam)
    wx, wy = R.ray_tables(60, 40, 500.0, 500.0, 29.5, 19.5)
    assert rx.dtype == np.int32 and np.array_equal(rx, wx) and np.array_equal(ry, wy)
    s = K.scaled_camera(P.Camera(640, 480, 520.0, 510.0, 319.5, 239.5), 4)
    assert (s.width, s.height, s.fx, s.fy, s.cx, s.cy) == (160, 120, 130.0, 127.5, 79.5, 59.5)
    assert K.scaled_camera(cam, 1) is cam
    q = P.projection_q8(P.Calibration(cam, P.Camera(640, 480, 520.0, 510.0, 319.5, 239.5), np.eye(3).tolist(), (0, 0, 0)), 4)
    assert q.tolist() == [int(round(256 * s.fx)), int(round(256 * s.fy)), int(round(256 * s.cx)), int(round(256 * s.cy))]


@pytest.mark.parametrize("cam, word", [
    ("a camera", "camera must be a register.Camera"),
    (P.Camera(60, 40, 500.0, 500.0, 29.5, 19.5, (0.1, 0, 0, 0, 0)), "dist .* is not zero.*undistort"),
    (P.Camera(60, 40, 7.0, 500.0, 29.5, 19.5), "a ray of 2\\^22 or more"),
    (P.Camera(60, 40, 500.0, 4.8, 29.5, 19.5), "a ray of 2\\^22 or more"),
])
def test_ray_tables_refusals(cam, word):
    with pytest.raises(ValueError, match="ray_tables: " + word):
        K.ray_tables(cam)


def test_ray_limit_is_exact():
    ok = P.Camera(5, 1, 1.0, 1.0, 4.0 - 2.0 ** -20, 0.0)              # RX[0] = -(2^22 - 1)
    assert K.ray_tables(ok)[0][0] == -(R.RAY_LIMIT - 1)
    with pytest.raises(ValueError, match="a ray of 2\\^22 or more"):
        K.ray_tables(P.Camera(5, 1, 1.0, 1.0, 4.0, 0.0))


@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("color", [False, True])
def test_ply_round_trip_and_header_bytes(tmp_path, normals, color):
    shape = R.SHAPES[2]
    rx, ry = R.tables(shape)
    rec, counts, _ = R.cloud_plane(R.plane(shape, "random")[0], rx, ry, normals=normals, color=R.tint(shape, 3)[0] if color else None)
    n = len(rec)
    head = K.ply_header(n, normals, color)
    want = ("ply\nformat binary_little_endian 1.0\ncomment x right, y down, z forward, in metres\n" + f"element vertex {n}\n"
            + "property float x\nproperty float y\nproperty float z\n"
            + ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "")
            + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if color else "") + "end_header\n")
    assert head == want.encode("ascii")
    assert K.record_size(normals, color) == rec.dtype.itemsize == K.record_dtype(normals, color).itemsize
    assert K.record_dtype(normals, color) == R.record_dtype(normals, color)
    path = str(tmp_path / "a.ply")
    K.write_ply(path, rec.tobytes() + b"\xee" * 40, n, normals, color)          # a body longer than the records: the prefix is written
    with open(path, "rb") as fh:
        assert fh.read() == head + rec.tobytes()
    back = K.read_ply(path)
    assert back.dtype == rec.dtype and back.tobytes() == rec.tobytes() and back["z"].base is not None
    K.write_ply(path, np.frombuffer(rec.tobytes(), dtype=np.uint8), n, normals, color)
    assert K.read_ply(path).tobytes() == rec.tobytes()
    K.write_ply(path, b"", 0, normals, color)
    assert len(K.read_ply(path)) == 0
    with pytest.raises(ValueError, match="write_ply: .* bytes of body"):
        K.write_ply(path, rec.tobytes()[:-1], n, normals, color)
    with open(path, "wb") as fh:
        fh.write(head + rec.tobytes()[:-1])
    with pytest.raises(ValueError, match="read_ply: .* bytes of body"):
        K.read_ply(path)
    with open(path, "wb") as fh:
        fh.write(head.replace(b"comment x right", b"comment x left") + rec.tobytes())
    with pytest.raises(ValueError, match="not the header codon_amd.cloud writes"):
        K.read_ply(path)
    with open(path, "wb") as fh:
        fh.write(b"P6\n1 1\n255\n")
    with pytest.raises(ValueError, match="is not a PLY file"):
        K.read_ply(path)
    with pytest.raises(ValueError, match="ply_header: count -1"):
        K.ply_header(-1, normals, color)


GOOD = P.Camera(**CAM)


@pytest.mark.parametrize("kw, word", [
    (dict(camera="cam"), "camera must be a register.Camera"),
    (dict(camera=P.Camera(60, 40, 500.0, 500.0, 29.5, 19.5, (0, 0, 1e-3, 0, 0))), "camera.dist .* is not zero: undistort the images first"),
    (dict(scale=2), "scale 2 "), (dict(scale=16, camera=P.Camera(60, 15, 500.0, 500.0, 29.5, 7.0)), "leaves nothing at scale 16"),
    (dict(depth_unit=0.0), "depth_unit 0.0 "), (dict(depth_unit=float("nan")), "depth_unit nan "), (dict(depth_unit="mm"), "depth_unit 'mm' "),
    (dict(radius=0), "radius 0 "), (dict(radius=9), "radius 9 "), (dict(radius=2.0), "radius 2.0 "),
    (dict(tolerance=-1), "tolerance -1 "), (dict(tolerance=65536), "tolerance 65536 "), (dict(tolerance=True), "tolerance True "),
    (dict(tolerance_rel=1.0), "tolerance_rel 1.0 "), (dict(tolerance_rel=-0.1), "tolerance_rel -0.1 "),
    (dict(camera=P.Camera(60, 40, 7.0, 500.0, 29.5, 19.5)), "a ray of 2\\^22 or more"),
])
def test_unprojection_refusals(kw, word):
    """Every refusal comes before the device is touched"""
    with pytest.raises(ValueError, match=word):
        K.Unprojection(**{"camera": GOOD, **kw})


def cloud_caller(lib, src, rx, ry, body, counts, ws, color=None, nmap=None, stream=None):
    """The good call of cloud_ref.REFUSALS -- u16 codes, a 5 x 7 plane, normals and RGB -- over the given addresses, with what a
    refusal changes as keyword arguments; shared with the GPU test"""
    P_ = C.c_void_p

    def call(B=1, h=5, w=7, src=src, fmt=L.FILL_U16, top=65535, rx=rx, ry=ry, span=(-100, 100, -90, 90), m=0.001 / (1 << 20), normals=1,
             radius=2, tol_abs=2, tol_rel=RQ, color=color, channels=3, body=body, counts=counts, nmap=None, ws=ws, ws_bytes=None):
        need = lib.codon_cloud_workspace_bytes(B, h, w)
        ws_bytes = need if ws_bytes is None else need - 1
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_cloud_points(B, h, w, p(src), fmt, top, p(rx), p(ry), None if span is None else (C.c_int32 * 4)(*span), m, normals,
                                    radius, tol_abs, tol_rel, p(color), channels, p(body), p(counts), p(body if nmap == "set" else nmap),
                                    p(ws), ws_bytes, stream)
        return st, lib.codon_last_error_string().decode()
    return call


def cloud_refusals(lib, call):
    for kw, word in R.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("cloud_points: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="cloud_points failed with status -1: cloud_points: "):
            L.check(st, "cloud_points")


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    q = lib.codon_cloud_workspace_bytes
    assert q(1, 5, 7) == 16 and q(3, 5, 7) == 48 and q(1, 32, 32) == 16 and q(1, 25, 41) == 16 and q(1, 65, 64) == 32
    assert q(1, 4096, 4096) == 16384 * 4 and q(2, 520, 512) == 2 * 260 * 4
    assert q(0, 5, 7) == 0 and q(65536, 5, 7) == 0 and q(1, 0, 7) == 0 and q(1, 5, 4097) == 0
    call = cloud_caller(lib, 4096, 8192, 12288, 16385, 20480, 24576, color=28673)  # never dereferenced: every call is refused on the host
    cloud_refusals(lib, call)
    for kw in ({"src": 4097}, {"rx": 8194}, {"ry": 12289}, {"counts": 20482}, {"ws": 24584}):
        assert "unaligned" in call(**kw)[1], kw
    # the body, the colour and the map need no alignment, and at the bounds themselves the refusal is the short workspace
    at = dict(top=10000, tol_abs=10000, tol_rel=65535, radius=8, span=(-(1 << 22) + 1, (1 << 22) - 1, 0, 0), ws_bytes="short")
    assert "too small" in call(**at)[1]
    assert "too small" in call(tol_abs=0, tol_rel=0, radius=1, normals=0, color=None, channels=0, m=5e-324, ws_bytes="short")[1]
    assert "too small" in call(nmap=32769, channels=1, ws_bytes="short")[1]


# ---- the command line ---------------------------------------------------------------------------------------------------------------

NEEDED = ["--depth", "d", "--calib", "c.json", "--out", "o"]


@pytest.mark.parametrize("argv, word", [
    (NEEDED[2:], "the following arguments are required: --depth"),
    (NEEDED[:2] + NEEDED[4:], "the following arguments are required: --calib"),
    (NEEDED[:4], "the following arguments are required: --out"),
    ([*NEEDED, "--depth-bits", "12"], "invalid choice"), ([*NEEDED, "--scale", "2"], "invalid choice"),
    ([*NEEDED, "--camera", "ir"], "invalid choice"),
    ([*NEEDED, "--depth-max", "10000"], "--depth-max needs --depth-bits 16"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "0"], "--depth-max 0 must be in \\[1, 65535\\]"),
    ([*NEEDED, "--depth-unit", "0"], "--depth-unit 0.0 must be positive"),
    ([*NEEDED, "--depth-unit", "nan"], "--depth-unit nan must be positive"),
    ([*NEEDED, "--color", "c", "--scale", "4"], "--color with --scale 4"),
    ([*NEEDED, "--no-normals", "--normal-maps", "n"], "--normal-maps needs normals"),
    ([*NEEDED, "--no-normals", "--normal-radius", "3"], "--normal-radius with --no-normals"),
    ([*NEEDED, "--no-normals", "--normal-tolerance-rel", "0.1"], "--normal-tolerance-rel with --no-normals"),
    ([*NEEDED, "--normal-radius", "0"], "--normal-radius 0 must be in \\[1, 8\\]"),
    ([*NEEDED, "--normal-radius", "9"], "--normal-radius 9 must be in \\[1, 8\\]"),
    ([*NEEDED, "--normal-tolerance", "-1"], "--normal-tolerance -1 must be in \\[0, 255\\]"),
    ([*NEEDED, "--normal-tolerance", "256"], "--normal-tolerance 256 must be in \\[0, 255\\]"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "10000", "--normal-tolerance", "10001"], "--normal-tolerance 10001 must be in \\[0, 10000\\]"),
    ([*NEEDED, "--normal-tolerance-rel", "1.0"], "--normal-tolerance-rel 1.0 must be in \\[0, 1\\)"),
    (["--depth", "d", "--calib", "c.json", "--out", "./d"], "--out is --depth"),
    ([*NEEDED, "--color", "o"], "--out is --color"),
    ([*NEEDED, "--normal-maps", "d/"], "--normal-maps is --depth or --color"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        K.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def _rig(tmp_path, name="rig.json", **changes):
    cam = dict(CAM)
    m = {"depth": dict(cam, **changes.get("depth", {})), "color": dict(cam, **changes.get("color", {})),
         "rotation": np.eye(3).tolist(), "translation": [0.0, 0.0, 0.0]}
    path = tmp_path / name
    path.write_text(json.dumps(m))
    return str(path)


def test_command_line_defaults_and_what_main_refuses_before_the_gpu(tmp_path, capsys):
    a, _ = K.parse_args(NEEDED)
    assert (a.camera, a.scale, a.depth_bits, a.depth_unit, a.normal_radius, a.normal_tolerance, a.normal_tolerance_rel) == \
        ("color", 1, 8, 0.001, 2, 2, 0.02) and not a.no_normals and not a.stats and a.color is None and a.normal_maps is None
    d = tmp_path / "d"
    d.mkdir()
    base = ["--depth", str(d), "--out", str(tmp_path / "o")]
    for argv, word in (
            ([*base, "--calib", str(tmp_path / "none.json")], "--calib .*none.json: "),
            (["--depth", str(tmp_path / "no"), "--out", str(tmp_path / "o"), "--calib", _rig(tmp_path)], "is not a directory"),
            ([*base, "--calib", _rig(tmp_path), "--color", str(tmp_path / "no")], "--color .* is not a directory"),
            ([*base, "--calib", _rig(tmp_path, "c.json", color={"dist": [0.1, 0, 0, 0, 0]})], "color.dist .* is not zero: undistort the colour images first"),
            ([*base, "--calib", _rig(tmp_path, "d.json", depth={"dist": [0.1, 0, 0, 0, 0]}), "--camera", "depth"], "depth.dist .* is not zero")):
        with pytest.raises(SystemExit) as e:
            K.main(argv)
        assert e.value.code == 2 and re.search(word, capsys.readouterr().err), argv
