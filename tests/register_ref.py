"""numpy restatement of the depth registration (codon_amd/csrc/register.hip, codon_amd.register) and the inputs
its tests share -- TEST INFRASTRUCTURE.  Integers only past the tables: the kernels are held to these bits, no tolerance.  A
DEFINITION of this project: a z-buffered forward projection of a depth sensor's map onto the colour camera's grid.

Inputs: codes c (B, hs, ws), 0 a hole, on the grid 1 .. top; the corner-ray table A, int32 (hs + 1, ws + 1, 3),
A[i][j] = rint(2^20 R r) with r the undistorted normalised ray of the source image point (j - 0.5, i - 0.5), the top-left corner
of pixel (i, j) -- (x_n, y_n, 1) for z-depth files, r / |r| for ranges along the ray -- and R the depth -> colour rotation; the
translation T = rint(2^20 t / unit), int64[3], in Q20 codes; the projection FX, FY, CX, CY, int32 in Q8 pixels of the output grid,
FX = rint(256 fx / s), CX = rint(256 ((cx + 0.5) / s - 0.5)); the output size (ho, wo).  The tables are float64 on the host, once;
the bounds |A| < 2^22, |T| < 2^38, 0 < FX, FY < 2^20, |CX|, |CY| < 2^21 keep every intermediate below 2^61.

A valid source pixel (i, j) with code k has the corners a = (i, j), b = (i + 1, j + 1), c = (i, j + 1), d = (i + 1, j);
P_q = k A[q] + T (int64).  Any P_q.z < 2^20: dropped.  z' = (((P_a.z + P_b.z + 1) >> 1) + 2^19) >> 20; not 1 <= z' <= top: dropped.
U_q = floor((FX P_q.x + CX P_q.z) / P_q.z), V_q likewise: Q8 pixel coordinates.  The footprint is the target pixels whose centre
lies in the half-open box of the four corners: x0 = (min U + 255) >> 8, x1 = ((max U + 255) >> 8) - 1, y likewise.  Wider or taller
than 8: dropped.  Empty: nothing is written (and nothing counted).  Wholly outside the plane: counted as outside.  Else it is
clipped to the plane and every pixel of it takes min(zbuf, z').  The output is the z-buffer where one was written, 0 elsewhere.
Statistics per image, four u32: valid source pixels, outside, dropped, filled target pixels."""
import functools

import numpy as np

Q = 20
ONE = 1 << Q
A_LIMIT, T_LIMIT, F_LIMIT, C_LIMIT = 1 << 22, 1 << 38, 1 << 20, 1 << 21
MAX_FOOT = 8
MAX_SIDE = 4096
UNDISTORT_ITERS = 40
CORNERS = ((0, 0), (1, 1), (0, 1), (1, 0))          # a, b, c, d as (di, dj)
STATS = ("valid", "outside", "dropped", "filled")


# ---- the tables: float64 on the host ------------------------------------------------------------------------------------------------

def distort(x, y, dist):
    """The Brown model (k1, k2, p1, p2, k3) on normalised coordinates"""
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return x * rad + dx, y * rad + dy


def undistort(xd, yd, dist):
    """The inverse of `distort` by UNDISTORT_ITERS fixed-point iterations x <- (x_d - tangential(x)) / radial(x)"""
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(UNDISTORT_ITERS):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
        x, y = (xd - dx) / rad, (yd - dy) / rad
    return x, y


def corner_rays(hs, ws, fx, fy, cx, cy, dist, radial=False):
    """(hs + 1, ws + 1, 3) float64: the undistorted rays of the pixels' corners, not rotated"""
    j, i = np.meshgrid(np.arange(ws + 1, dtype=np.float64), np.arange(hs + 1, dtype=np.float64))
    x, y = undistort((j - 0.5 - cx) / fx, (i - 0.5 - cy) / fy, tuple(float(d) for d in dist))
    r = np.stack([x, y, np.ones_like(x)], axis=-1)
    if radial:
        r = r / np.sqrt((r * r).sum(axis=-1, keepdims=True))
    return r


def ray_table(hs, ws, fx, fy, cx, cy, dist, rot, radial=False):
    r = corner_rays(hs, ws, fx, fy, cx, cy, dist, radial)
    a = np.rint(float(ONE) * (r @ np.asarray(rot, dtype=np.float64).T))
    assert np.abs(a).max() < A_LIMIT
    return a.astype(np.int32)


def translation_q20(t, unit):
    v = np.rint(float(ONE) * np.asarray(t, dtype=np.float64) / float(unit))
    assert np.abs(v).max() < T_LIMIT
    return v.astype(np.int64)


def projection_q8(fx, fy, cx, cy, s):
    p = [np.rint(256.0 * fx / s), np.rint(256.0 * fy / s), np.rint(256.0 * ((cx + 0.5) / s - 0.5)), np.rint(256.0 * ((cy + 0.5) / s - 0.5))]
    assert 0 < p[0] < F_LIMIT and 0 < p[1] < F_LIMIT and abs(p[2]) < C_LIMIT and abs(p[3]) < C_LIMIT
    return np.array(p, dtype=np.int32)


# ---- the definition: integers -------------------------------------------------------------------------------------------------------

def project(c, A, T, proj, top):
    """Of one plane: (U, V) int64 (4, hs, ws) of the corners a, b, c, d in Q8 pixels (0 where not kept), z' int64 (hs, ws),
    valid, kept (bool): kept = valid, every corner in front of the camera, z' on the grid"""
    c = np.asarray(c).astype(np.int64)
    hs, ws = c.shape
    A = np.asarray(A).astype(np.int64)
    assert A.shape == (hs + 1, ws + 1, 3) and np.abs(A).max() < A_LIMIT
    T = np.asarray(T).astype(np.int64)
    FX, FY, CX, CY = (int(v) for v in proj)
    valid = c != 0
    P = [c[:, :, None] * A[di:di + hs, dj:dj + ws] + T for di, dj in CORNERS]
    front = np.ones_like(valid)
    for p in P:
        front &= p[..., 2] >= ONE
    z = (((P[0][..., 2] + P[1][..., 2] + 1) >> 1) + (ONE >> 1)) >> Q
    kept = valid & front & (z >= 1) & (z <= top)
    U = np.zeros((4, hs, ws), dtype=np.int64)
    V = np.zeros((4, hs, ws), dtype=np.int64)
    for q, p in enumerate(P):
        pz = np.where(kept, p[..., 2], 1)
        U[q] = np.where(kept, (FX * p[..., 0] + CX * p[..., 2]) // pz, 0)
        V[q] = np.where(kept, (FY * p[..., 1] + CY * p[..., 2]) // pz, 0)
    return U, V, z, valid, kept


def splat(U, V, z, valid, kept, ho, wo):
    """The z-buffer of one plane from the corners' coordinates (any number of corners: the box of them) -> (out int64 (ho, wo),
    0 where nothing was written, stats int64[4], the dropped count's part that is an oversize footprint)"""
    x0, x1 = (U.min(axis=0) + 255) >> 8, ((U.max(axis=0) + 255) >> 8) - 1
    y0, y1 = (V.min(axis=0) + 255) >> 8, ((V.max(axis=0) + 255) >> 8) - 1
    over = kept & ((x1 - x0 + 1 > MAX_FOOT) | (y1 - y0 + 1 > MAX_FOOT))
    live = kept & ~over & (x1 >= x0) & (y1 >= y0)
    outside = live & ((x1 < 0) | (x0 >= wo) | (y1 < 0) | (y0 >= ho))
    live &= ~outside
    big = np.iinfo(np.int64).max
    zb = np.full(ho * wo, big, dtype=np.int64)
    ii, jj = np.nonzero(live)
    X0, X1, Y0, Y1, Z = x0[ii, jj], x1[ii, jj], y0[ii, jj], y1[ii, jj], z[ii, jj]
    for dy in range(MAX_FOOT):
        for dx in range(MAX_FOOT):
            y, x = Y0 + dy, X0 + dx
            ok = (y <= Y1) & (x <= X1) & (y >= 0) & (y < ho) & (x >= 0) & (x < wo)
            np.minimum.at(zb, (y * wo + x)[ok], Z[ok])
    out = np.where(zb == big, 0, zb).reshape(ho, wo)
    stats = np.array([valid.sum(), outside.sum(), (valid & ~kept).sum() + over.sum(), (zb != big).sum()], dtype=np.int64)
    return out, stats, int(over.sum())


def register_plane(c, A, T, proj, ho, wo, top):
    """(out (ho, wo) in the plane's dtype, stats uint32[4])"""
    c = np.asarray(c)
    U, V, z, valid, kept = project(c, A, T, proj, top)
    out, stats, _ = splat(U, V, z, valid, kept, ho, wo)
    res = out.astype(c.dtype)
    assert np.array_equal(res, out)
    return res, stats.astype(np.uint32)


def register(c, A, T, proj, ho, wo, top):
    """register_plane over a (B, hs, ws) batch -> ((B, ho, wo) codes, (B, 4) uint32)"""
    r = [register_plane(p, A, T, proj, ho, wo, top) for p in np.asarray(c)]
    return np.stack([o for o, _ in r]), np.stack([s for _, s in r])


def cracks(out):
    """The holes with filled neighbours left and right, or above and below"""
    f = np.asarray(out) != 0
    n = np.zeros(f.shape, dtype=bool)
    n[:, 1:-1] |= ~f[:, 1:-1] & f[:, :-2] & f[:, 2:]
    n[1:-1] |= ~f[1:-1] & f[:-2] & f[2:]
    return int(n.sum())


def rotation(rx, ry, rz):
    """Rz(rz) Ry(ry) Rx(rx), radians"""
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


# ---- the shared cases of the GPU test and of the host-side check ----------------------------------------------------------------------

# (B, hs, ws, ho, wo, scale, colour height, colour width): the smallest at which each part can go wrong -- one pixel; odd sizes; exactly
# one 16 x 16 tile; one pixel past a tile on both axes onto a finer grid (footprints of 2 - 3); a batch onto a coarser grid (empty
# footprints); several tiles at scale 4 from a colour image that (ho, wo) = (H // s, W // s) leaves no remainder of
SHAPES = ((1, 1, 1, 1, 1, 1, 1, 1), (1, 5, 7, 3, 5, 1, 3, 5), (1, 16, 16, 16, 16, 1, 16, 16), (1, 17, 33, 40, 80, 1, 40, 80),
          (3, 24, 32, 12, 16, 1, 12, 16), (1, 70, 130, 35, 65, 4, 140, 260))
FORMATS = (("u8", 255), ("u16", 65535), ("u16_10000", 10000))
PATTERNS = ("random", "all", "none", "scene", "near")
CALIBS = ("identity", "translation", "mixed", "half_outside")
RANGE_M = 2.5               # the metres the grid 1 .. top spans in the cases: unit = RANGE_M / top
T_TRANSLATION = (0.01, -0.005, -0.3)     # the colour camera well in front: the near pattern lives in the 0.3 m it steps over
T_MIXED = (-0.04, 0.02, 0.03)
DIST_MIXED = (-0.3, 0.1, 1e-3, 1e-3, 0.0)


def unit_of(top):
    return RANGE_M / top


@functools.lru_cache(maxsize=None)
def calibration(shape, calib):
    """A rig for a shape, as the mapping codon_amd.register.Calibration.from_mapping reads: the depth camera sees about 50 degrees,
    the colour camera the same field on its own grid"""
    _, hs, ws, ho, wo, s, Hc, Wc = shape
    fd = 1.1 * max(hs, ws)
    depth = dict(width=ws, height=hs, fx=fd, fy=fd * 1.01, cx=(ws - 1) / 2 + 0.3, cy=(hs - 1) / 2 - 0.2, dist=[0.0] * 5)
    fc = fd * Wc / ws
    color = dict(width=Wc, height=Hc, fx=fc, fy=fc * 1.01 * (Hc / hs) / (Wc / ws), cx=(Wc - 1) / 2, cy=(Hc - 1) / 2, dist=[0.0] * 5)
    rot, t = np.eye(3), (0.0, 0.0, 0.0)
    if calib == "translation":
        t = T_TRANSLATION
    elif calib == "mixed":
        rot, t = rotation(-0.03, 0.05, 0.1), T_MIXED
        depth["dist"] = list(DIST_MIXED)
    elif calib == "half_outside":
        color["cx"] = color["cx"] + Wc / 2
        t = (0.0, 0.01, 0.0)
    else:
        assert calib == "identity"
    return dict(depth=depth, color=color, rotation=[[float(v) for v in row] for row in rot], translation=list(t))


@functools.lru_cache(maxsize=None)
def tables(shape, calib, top):
    """(A, T, proj) of a case, read-only"""
    _, hs, ws, ho, wo, s, Hc, Wc = shape
    m = calibration(shape, calib)
    d, c = m["depth"], m["color"]
    A = ray_table(hs, ws, d["fx"], d["fy"], d["cx"], d["cy"], d["dist"], m["rotation"])
    T = translation_q20(m["translation"], unit_of(top))
    P = projection_q8(c["fx"], c["fy"], c["cx"], c["cy"], s)
    for a in (A, T, P):
        a.setflags(write=False)
    assert (Hc // s, Wc // s) == (ho, wo)
    return A, T, P


@functools.lru_cache(maxsize=None)
def plane(shape, pattern, top, seed=1):
    """(B, hs, ws) codes of a pattern, u8 for top 255 and u16 otherwise, read-only"""
    B, hs, ws = shape[:3]
    g = np.random.default_rng([seed, B, hs, ws, top, PATTERNS.index(pattern)])
    dt = np.uint8 if top == 255 else np.uint16
    if pattern == "random":                 # 20 % holes, codes over the grid's upper three quarters, top itself among them
        c = g.integers(top // 4, top + 1, size=(B, hs, ws))
        c[g.random((B, hs, ws)) < 0.2] = 0
        c.flat[0] = top
    elif pattern == "all":
        c = np.zeros((B, hs, ws), dtype=np.int64)
    elif pattern == "none":
        c = g.integers(top // 4, top + 1, size=(B, hs, ws))
    elif pattern == "scene":                # a background, and a foreground square in the middle third
        c = np.full((B, hs, ws), 3 * top // 4, dtype=np.int64)
        c[:, hs // 3:hs // 3 + max(1, hs // 3), ws // 3:ws // 3 + max(1, ws // 3)] = top // 4
    else:                                   # a plane so near that the translated rigs magnify a pixel beyond 8, or see it behind them
        assert pattern == "near"
        tz = -T_TRANSLATION[2] / unit_of(top)                           # z' = k - tz there: a pixel is magnified k / (k - tz) times,
        f = np.geomspace(0.02, 1.0, ws)                                 # from 50 times on the left to 2 times on the right
        c = np.ceil(tz * (1.0 + f))[None, None, :].astype(np.int64) + g.integers(0, 2, size=(B, hs, ws))
    out = c.astype(dt)
    assert np.array_equal(out, c)
    out.setflags(write=False)
    return out


def cases(shape):
    """[(format name, top, pattern, calibration)] of a shape: every pattern under every calibration, the formats in turn -- a
    shape sees every format, pattern and calibration, and a pattern under a calibration every format over the shapes"""
    si = SHAPES.index(tuple(shape))
    return [(*FORMATS[(pi + ci + si) % 3], pattern, calib) for pi, pattern in enumerate(PATTERNS) for ci, calib in enumerate(CALIBS)]


@functools.lru_cache(maxsize=None)
def want(shape, pattern, top, calib, seed=1):
    """(codes, stats) of a case, computed once, read-only"""
    A, T, P = tables(shape, calib, top)
    out, stats = register(plane(shape, pattern, top, seed), A, T, P, shape[3], shape[4], top)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


# codon_register_depth's refusals: (what differs from a good call of u16 codes, a 5 x 7 source onto 3 x 5, a piece of the message)
REFUSALS = [({"src": None}, "null pointer"), ({"out": None}, "null pointer"), ({"ws": None}, "null pointer"),
            ({"rays": None}, "null pointer"), ({"trans": None}, "null pointer"), ({"proj": None}, "null pointer"),
            ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "), ({"B": 0}, "batch 0 "), ({"B": 65536}, "batch 65536 "),
            ({"hs": 0}, "a 0x7 source"), ({"ws_": 0}, "a 5x0 source"), ({"hs": 4097}, "a 4097x7 source"), ({"ws_": 4097}, "a 5x4097 source"),
            ({"ho": 0}, "a 0x5 target"), ({"wo": 4097}, "a 3x4097 target"), ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "),
            ({"fmt": 0, "top": 1000}, "top 1000 "),
            ({"T": (T_LIMIT, 0, 0)}, "translation"), ({"T": (0, -T_LIMIT, 0)}, "translation"), ({"T": (0, 0, T_LIMIT)}, "translation"),
            ({"P": (F_LIMIT, 256, 0, 0)}, "projection"), ({"P": (256, F_LIMIT, 0, 0)}, "projection"), ({"P": (0, 256, 0, 0)}, "projection"),
            ({"P": (256, -1, 0, 0)}, "projection"), ({"P": (256, 256, C_LIMIT, 0)}, "projection"), ({"P": (256, 256, 0, -C_LIMIT)}, "projection"),
            ({"out": "src"}, "same buffer"), ({"ws_bytes": "short"}, "too small")]
