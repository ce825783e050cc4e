"""numpy restatement of the point clouds with normals (codon_amd/csrc/cloud.hip, codon_amd.cloud) and the inputs its
tests share -- TEST INFRASTRUCTURE.  The kernels are held to these bytes, no tolerance.  A DEFINITION of this project.

Tables, float64, once: RX[j] = rint(2^20 (j - cx) / fx), RY[i] = rint(2^20 (i - cy) / fy), int32, |RX|, |RY| < 2^22.
A valid pixel (i, j), code k, 1 <= k <= 65535: P = (k RX[j], k RY[i], k << 20), int64 Q20 codes; the record holds
float32(float64(P_c) m) with m = depth_unit / 2^20: one multiply in double, one conversion.
Normal, radius R: P8 = (P + 2^11) >> 12.  Along x the far pixels are (i, j + R) ahead and (i, j - R) behind, along y (i + R, j)
and (i - R, j); a far pixel COUNTS if inside the plane and linked to k under clean's rule with A' = R A and Rq.  Tangent:
P8+ - P8- (both), P8+ - P8 (ahead only), P8 - P8- (behind only); neither, on either axis: no normal.  n = du x dv in int64;
s = max(0, bitlength(max |n_c|) - 30), n_c <- sign(n_c) (|n_c| >> s); L = isqrt(n . n), L = 0: no normal; n . P8 > 0: n negated;
N_c = floor((2 n_c 16384 + L) / (2 L)); the record holds float32(N_c) 2^-14, three zeros without a normal.
Records: x y z [nx ny nz] [r g b], little-endian, packed, one per non-zero code in row-major order.  Normal map: channel
128 + ((127 N_c + 8192) >> 14), (0, 0, 0) for a hole or a pixel without a normal.  Counts: records, records with a normal."""
import functools
import math

import numpy as np

from tests.clean_ref import linked, rel_q16

MAX_SIDE, MAX_RADIUS, RAY_LIMIT, ONE = 4096, 8, 1 << 22, 16384
RUN = 1024                                  # CD_RUN of codon_amd/csrc/cloud_tile.h
DEFAULTS = dict(depth_unit=0.001, radius=2, tolerance=2, tolerance_rel=0.02)


def ray_tables(width, height, fx, fy, cx, cy):
    """RX (width), RY (height), int32"""
    rx = np.rint(float(1 << 20) * (np.arange(width, dtype=np.float64) - cx) / fx)
    ry = np.rint(float(1 << 20) * (np.arange(height, dtype=np.float64) - cy) / fy)
    assert max(np.abs(rx).max(), np.abs(ry).max()) < RAY_LIMIT
    return rx.astype(np.int32), ry.astype(np.int32)


def record_dtype(normals, color):
    f = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    if normals:
        f += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
    if color:
        f += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    return np.dtype(f)                      # packed: 12, 24, 15 or 27 bytes


def points_q20(c, rx, ry):
    """P: (h, w, 3) int64 of (h, w) codes"""
    k = np.asarray(c).astype(np.int64)
    return np.stack([k * rx.astype(np.int64)[None, :], k * ry.astype(np.int64)[:, None], k << 20], axis=-1)


def _far(a, di, dj):
    """a[i + di, j + dj], 0 outside the plane (a: (h, w) or (h, w, 3))"""
    h, w = a.shape[:2]
    out = np.zeros_like(a)
    ys, yd = (slice(di, h), slice(0, h - di)) if di >= 0 else (slice(0, h + di), slice(-di, h))
    xs, xd = (slice(dj, w), slice(0, w - dj)) if dj >= 0 else (slice(0, w + dj), slice(-dj, w))
    if abs(di) < h and abs(dj) < w:
        out[yd, xd] = a[ys, xs]
    return out


def tangent(k, p8, di, dj, A, Rq):
    """(d (h, w, 3) int64, ok (h, w)) along (di, dj): the far pixels are (i + di, j + dj) and (i - di, j - dj)"""
    fa, fb = linked(k, _far(k, di, dj), A, Rq), linked(k, _far(k, -di, -dj), A, Rq)
    hi = np.where(fa[..., None], _far(p8, di, dj), p8)
    lo = np.where(fb[..., None], _far(p8, -di, -dj), p8)
    return hi - lo, fa | fb


def bitlength(v):
    """of a non-negative int64 array"""
    return sum(((v >> b) != 0).astype(np.int64) for b in range(63))


def isqrt(v):
    return np.array([math.isqrt(int(x)) for x in v.ravel()], dtype=np.int64).reshape(v.shape)


def normals_q14(c, rx, ry, radius, tolerance, tolerance_rel_q16):
    """(N (h, w, 3) int64 in Q14, has (h, w) bool) of (h, w) codes; N is 0 where has is not set"""
    k = np.asarray(c).astype(np.int64)
    p8 = (points_q20(k, rx, ry) + 2048) >> 12
    A = radius * tolerance
    du, okx = tangent(k, p8, 0, radius, A, tolerance_rel_q16)
    dv, oky = tangent(k, p8, radius, 0, A, tolerance_rel_q16)
    n = np.stack([du[..., 1] * dv[..., 2] - du[..., 2] * dv[..., 1], du[..., 2] * dv[..., 0] - du[..., 0] * dv[..., 2],
                  du[..., 0] * dv[..., 1] - du[..., 1] * dv[..., 0]], axis=-1)
    s = np.maximum(0, bitlength(np.abs(n).max(axis=-1)) - 30)[..., None]
    n = np.sign(n) * (np.abs(n) >> s)
    L = isqrt((n * n).sum(axis=-1))
    n = np.where(((n * p8).sum(axis=-1) > 0)[..., None], -n, n)
    has = (k != 0) & okx & oky & (L > 0)
    Ls = np.where(has, L, 1)[..., None]
    N = np.where(has[..., None], (2 * n * ONE + Ls) // (2 * Ls), 0)
    return N, has


def cloud_plane(c, rx, ry, depth_unit=0.001, normals=True, radius=2, tolerance=2, tolerance_rel_q16=1311, color=None):
    """(records: a structured array, one per non-zero code in row-major order; counts: uint32 (2); normal map (h, w, 3) u8 or None)
    of one (h, w) plane; color: None, (h, w) or (h, w, 3) u8"""
    c = np.asarray(c)
    c = c.view(np.uint16) if c.dtype == np.int16 else c
    valid = c != 0
    P = points_q20(c, rx, ry)[valid]
    rec = np.zeros(len(P), dtype=record_dtype(normals, color is not None))
    m = float(depth_unit) / float(1 << 20)
    for q, name in enumerate("xyz"):
        rec[name] = (P[:, q].astype(np.float64) * m).astype(np.float32)
    counts, nmap = np.array([len(P), 0], dtype=np.uint32), None
    if normals:
        N, has = normals_q14(c, rx, ry, radius, tolerance, tolerance_rel_q16)
        for q, name in enumerate(("nx", "ny", "nz")):
            rec[name] = N[valid][:, q].astype(np.float32) * np.float32(1.0 / ONE)
        counts[1] = has.sum()
        nmap = np.where(has[..., None], 128 + ((127 * N + ONE // 2) >> 14), 0).astype(np.uint8)
    if color is not None:
        rgb = np.asarray(color)
        rgb = np.broadcast_to(rgb[..., None], (*rgb.shape, 3)) if rgb.ndim == 2 else rgb
        for q, name in enumerate(("red", "green", "blue")):
            rec[name] = rgb[valid][:, q]
    return rec, counts, nmap


def cloud(c, rx, ry, **kw):
    """cloud_plane over a (B, h, w) batch (color: (B, h, w[, 3])) -> ([records], (B, 2) uint32, (B, h, w, 3) u8 or None)"""
    color = kw.pop("color", None)
    r = [cloud_plane(p, rx, ry, color=None if color is None else color[b], **kw) for b, p in enumerate(np.asarray(c))]
    maps = None if r[0][2] is None else np.stack([x[2] for x in r])
    return [x[0] for x in r], np.stack([x[1] for x in r]), maps


# ---- scenes ----------------------------------------------------------------------------------------------------------------------------

def slanted_plane(top, z0, h=40, w=60, fx=500.0, fy=500.0, cx=29.5, cy=19.5):
    """codes of the plane Z = z0 / (1 - 0.5 x_n) in codes, rounded, and its analytic unit normal facing the camera"""
    xn = (np.arange(w, dtype=np.float64) - cx) / fx
    c = np.rint(np.broadcast_to(z0 / (1.0 - 0.5 * xn), (h, w)))
    assert c.min() >= 1 and c.max() <= top
    # Z (1 - 0.5 X / Z) = z0  <=>  Z - 0.5 X = z0: the plane's normal is (-0.5, 0, 1) / |.|, towards the camera (0.5, 0, -1) / |.|
    n = np.array([0.5, 0.0, -1.0]) / math.sqrt(1.25)
    return c.astype(np.uint8 if top == 255 else np.uint16), n


def two_surfaces(top, h=24, w=40, edge=20, near=None, far=None):
    """A near surface left of column `edge` and a far one right of it, both fronto-parallel, far more than any tolerance apart"""
    near = top // 5 if near is None else near
    far = 3 * (top // 5) if far is None else far
    c = np.full((h, w), far, dtype=np.int64)
    c[:, :edge] = near
    return c.astype(np.uint8 if top == 255 else np.uint16)


# ---- the shared cases of the GPU test and of the host-side check ----------------------------------------------------------------------

# (B, h, w): one pixel; a single row; odd sizes; exactly one block of 1024; a second block that holds one pixel; a batch, for the
# per-image offsets; many blocks with rows that are not aligned; 260 blocks, so a scan thread takes more than one block word
SHAPES = ((1, 1, 1), (1, 1, 37), (1, 5, 7), (1, 32, 32), (1, 25, 41), (3, 9, 33), (1, 93, 116), (1, 520, 512))
PATTERNS = ("random", "all", "none", "last", "checker", "surfaces", "high", "u8")
# (name, normals, colour channels (0: none), radius, tolerance or None for the top's own, normal map)
FORMS = (("xyz", False, 0, 2, None, False), ("normals", True, 0, 2, None, True), ("grey", False, 1, 2, None, False),
         ("full", True, 3, 2, None, True), ("full_grey_r1", True, 1, 1, None, False), ("r8", True, 0, 8, None, True),
         ("abs_0", True, 3, 2, 0, False))
BIG = SHAPES[7]
BIG_CASES = (("random", "full"), ("all", "normals"), ("last", "xyz"), ("surfaces", "r8"))    # of the 520 x 512 plane


def top_of(pattern):
    return 255 if pattern == "u8" else 65535 if pattern == "high" else 10000


def camera_of(shape):
    """(fx, fy, cx, cy) of a shape's camera: off-centre, not square"""
    _, h, w = shape
    return 0.9 * max(h, w) + 3.0, 0.8 * max(h, w) + 5.0, 0.45 * w + 0.25, 0.55 * h - 0.125


@functools.lru_cache(maxsize=None)
def tables(shape):
    _, h, w = shape
    rx, ry = ray_tables(w, h, *camera_of(shape))
    rx.setflags(write=False), ry.setflags(write=False)
    return rx, ry


def params(form, top):
    """(normals, channels, radius, A, Rq, normal map) of a form on a grid"""
    name, normals, channels, radius, A, nmap = next(f for f in FORMS if f[0] == form)
    return normals, channels, radius, max(2, top // 500) if A is None else A, rel_q16(DEFAULTS["tolerance_rel"]), nmap


@functools.lru_cache(maxsize=None)
def plane(shape, pattern, seed=1):
    """(B, h, w) codes of a pattern, u8 for the u8 pattern and u16 otherwise, read-only"""
    B, h, w = shape
    top = top_of(pattern)
    g = np.random.default_rng([seed, B, h, w, PATTERNS.index(pattern)])
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if pattern in ("random", "u8"):         # 30 % holes; a smooth surface with a few codes of noise, and a nearer half
        z = top // 2 + (top // 50) * np.sin(0.2 * i + 0.1) * np.cos(0.15 * j) + g.integers(-1, 2, size=shape)
        z = np.where(j[None] > w // 2, z // 2, z)
        c = np.where(g.uniform(size=shape) < 0.3, 0, np.clip(np.rint(z), 1, top)).astype(np.int64)
    elif pattern == "high":                 # codes of 32768 and above: an int16 view is negative
        c = np.where(g.uniform(size=shape) < 0.3, 0, 40000 + 40 * i + 25 * j + g.integers(-2, 3, size=shape)).astype(np.int64)
        c.flat[0] = 65535
    elif pattern == "all":
        c = np.broadcast_to(top // 2 + 3 * i + 2 * j, shape).astype(np.int64)
    elif pattern == "none":
        c = np.zeros(shape, dtype=np.int64)
    elif pattern == "last":
        c = np.zeros(shape, dtype=np.int64)
        c[:, -1, -1] = top // 3
    elif pattern == "checker":              # every other pixel a hole: the pixels 2 steps away are valid, those 1 step away are not
        c = np.broadcast_to(np.where((i + j) % 2 == 0, top // 4 + i, 0), shape).astype(np.int64)
    else:
        assert pattern == "surfaces"
        c = np.broadcast_to(two_surfaces(top, h, w, w // 2).astype(np.int64), shape)
    out = np.clip(c, 0, top).astype(np.uint8 if top == 255 else np.uint16)
    assert out.shape == shape
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tint(shape, channels):
    B, h, w = shape
    g = np.random.default_rng([7, B, h, w, channels])
    out = g.integers(0, 256, size=(B, h, w, 3) if channels == 3 else (B, h, w), dtype=np.uint8)
    out.setflags(write=False)
    return out


def cases(shape):
    """[(pattern, form)] of a shape: every pattern under every form, but the 520 x 512 plane under BIG_CASES alone"""
    if tuple(shape) == BIG:
        return list(BIG_CASES)
    return [(pattern, form[0]) for pattern in PATTERNS for form in FORMS]


@functools.lru_cache(maxsize=None)
def want(shape, pattern, form):
    """(body bytes per image [bytes], counts (B, 2) uint32, normal maps (B, h, w, 3) or None, rec) of a case, computed once"""
    normals, channels, radius, A, Rq, nmap = params(form, top_of(pattern))
    rx, ry = tables(shape)
    recs, counts, maps = cloud(plane(shape, pattern), rx, ry, depth_unit=DEFAULTS["depth_unit"], normals=normals, radius=radius,
                               tolerance=A, tolerance_rel_q16=Rq, color=tint(shape, channels) if channels else None)
    counts.setflags(write=False)
    return tuple(r.tobytes() for r in recs), counts, maps if nmap else None, record_dtype(normals, channels != 0).itemsize


# codon_cloud_points' refusals: (what differs from a good call of u16 codes on a 5 x 7 plane, a piece of the message)
REFUSALS = [({"src": None}, "null pointer"), ({"rx": None}, "null pointer"), ({"ry": None}, "null pointer"),
            ({"span": None}, "null pointer"), ({"body": None}, "null pointer"), ({"counts": None}, "null pointer"),
            ({"ws": None}, "null pointer"),
            ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "), ({"B": 0}, "batch 0 "), ({"B": 65536}, "batch 65536 "),
            ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"), ({"h": 4097}, "a 4097x7 plane"), ({"w": 4097}, "a 5x4097 plane"),
            ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "), ({"fmt": 0, "top": 1000}, "top 1000 "),
            ({"normals": 2}, "normals 2 "), ({"radius": 0}, "radius 0 "), ({"radius": 9}, "radius 9 "),
            ({"tol_abs": -1}, "tolerance -1 "), ({"top": 10000, "tol_abs": 10001}, "tolerance 10001 "),
            ({"tol_rel": -1}, "tolerance_rel -1 "), ({"tol_rel": 65536}, "tolerance_rel 65536 "),
            ({"span": (0, 1 << 22, 0, 0)}, "ray 1 of the span is 4194304"), ({"span": (0, 0, -(1 << 22), 0)}, "ray 2 of the span is -4194304"),
            ({"m": 0.0}, "m 0 "), ({"m": -1e-9}, "m -1e-09 "), ({"m": float("inf")}, "m inf "), ({"m": float("nan")}, "m nan "),
            ({"channels": 2}, "color_channels 2 "), ({"color": None, "channels": 3}, "color_channels 3 "),
            ({"normals": 0, "nmap": "set"}, "a normal map without normals"), ({"ws_bytes": "short"}, "too small")]
