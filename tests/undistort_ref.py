"""numpy restatement of the undistortion of colour images (codon_amd/csrc/undistort.hip, codon_amd.undistort) and the
inputs its tests share -- TEST INFRASTRUCTURE.  Integers only past the tables: the kernel is held to these bits, no tolerance.  A
DEFINITION of this project: the image of a camera with Brown distortion, resampled to a pinhole camera by a Catmull-Rom cubic.

Cameras are tuples (width, height, fx, fy, cx, cy, dist), pixel centres at integer coordinates.  src is the camera as calibrated,
dst a pinhole camera (dist zero).  Images are u8 (B, H, W, C) interleaved, C 1 or 3.

The map table M, int32 (ho, wo, 2): for the target pixel (i, j), x = (j - dst.cx) / dst.fx, y = (i - dst.cy) / dst.fy,
(xd, yd) = distort(x, y, src.dist), u = src.fx xd + src.cx, v = src.fy yd + src.cy, U = rint(32 u), V = rint(32 v): Q5 source pixels.
A pixel is OUTSIDE -- its entry (-2^20, -2^20) -- if U or V is not finite, U < -16 or U >= 32 W - 16 (V against H), r2 = x^2 + y^2
> 16, or r2 >= r2_fold: the first rho on the grid n / 4096, n = 0 .. 65536, with 1 + 3 k1 rho + 5 k2 rho^2 + 7 k3 rho^3 <= 0, where
the radial model (the tangential terms ignored) stops increasing; infinite if there is none.

The weight table K, int16 (32, 4): rint(2048 keys(p / 32)) at the taps -1, 0, 1, 2 (Keys, a = -0.5), the first of the largest
entries of a row adjusted so that every row sums to 2048.

A pixel that is not outside: xi = U >> 5, px = U & 31, yi and py likewise (arithmetic shifts); tap (r, c) is
src[clamp(yi - 1 + r)][clamp(xi - 1 + c)]; row_r = sum_c K[px][c] tap, acc = sum_r K[py][r] row_r, out = clamp((acc + 2^21) >> 22,
0, 255) per channel.  An outside pixel is 0 in every channel.

The tile table, int32 (ty, tx, 4) = kind, x0, y0, 0 per 32 x 8 tile of target pixels: EMPTY (no pixel inside), STAGED (the box of all
taps of the inside pixels, x0 = min xi - 1 .. max xi + 2 and y likewise, fits 48 x 24), DIRECT (everything else; x0 = y0 = 0 as
for EMPTY).  Counts: staged, direct, empty tiles, outside pixels."""
import functools

import numpy as np

OUTSIDE = -(1 << 20)
TILE_W, TILE_H = 32, 8
WIN_W, WIN_H = 48, 24
EMPTY, STAGED, DIRECT = 0, 1, 2
COUNTS = ("staged", "direct", "empty", "outside")
MAX_SIDE = 4096


# ---- the tables: float64 on the host ------------------------------------------------------------------------------------------------

def distort(x, y, dist):
    """The Brown model (k1, k2, p1, p2, k3) on normalised coordinates"""
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    dx = 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
    dy = p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return x * rad + dx, y * rad + dy


def r2_fold(dist):
    k1, k2, _, _, k3 = dist
    rho = np.arange(65537, dtype=np.float64) / 4096.0
    d = 1.0 + 3.0 * k1 * rho + 5.0 * k2 * rho * rho + 7.0 * k3 * rho * rho * rho
    at = np.flatnonzero(d <= 0.0)
    return float(rho[at[0]]) if at.size else float("inf")


def out_camera(src, focal_scale=1.0):
    w, h, fx, fy, cx, cy, _ = src
    return (w, h, fx * focal_scale, fy * focal_scale, cx, cy, (0.0,) * 5)


def map_table(src, dst, fold=True):
    """M; fold=False leaves the fold rule out (what the rule is for: test_undistort_cpu)"""
    W, H, sfx, sfy, scx, scy, dist = src
    wo, ho, dfx, dfy, dcx, dcy, _ = dst
    j, i = np.meshgrid(np.arange(wo, dtype=np.float64), np.arange(ho, dtype=np.float64))
    x, y = (j - dcx) / dfx, (i - dcy) / dfy
    xd, yd = distort(x, y, dist)
    with np.errstate(invalid="ignore", over="ignore"):
        U, V = np.rint(32.0 * (sfx * xd + scx)), np.rint(32.0 * (sfy * yd + scy))
        r2 = x * x + y * y
        out = ~np.isfinite(U) | ~np.isfinite(V) | (U < -16) | (U >= 32 * W - 16) | (V < -16) | (V >= 32 * H - 16) | (r2 > 16.0)
        if fold:
            out |= r2 >= r2_fold(dist)
    M = np.stack([np.where(out, OUTSIDE, U), np.where(out, OUTSIDE, V)], axis=-1)
    return M.astype(np.int32)


def keys(t):
    """The Keys cubic, a = -0.5"""
    t = np.abs(t)
    return np.where(t <= 1.0, (1.5 * t - 2.5) * t * t + 1.0, np.where(t < 2.0, ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0, 0.0))


@functools.lru_cache(maxsize=None)
def _weights():
    p = np.arange(32, dtype=np.float64)[:, None] / 32.0
    K = np.rint(2048.0 * keys(p - np.array([-1.0, 0.0, 1.0, 2.0])[None, :])).astype(np.int64)
    for row in K:
        row[int(np.argmax(row))] += 2048 - int(row.sum())          # argmax: the first of the largest
    return K.astype(np.int16)


def weight_table():
    return _weights().copy()


def tile_table(M, stage=True):
    """(tiles int32 (ty, tx, 4), counts uint32[4]); stage=False: the build with staging compiled out, every non-empty tile DIRECT"""
    ho, wo = M.shape[:2]
    ty, tx = -(-ho // TILE_H), -(-wo // TILE_W)
    tiles = np.zeros((ty, tx, 4), dtype=np.int32)
    n = [0, 0, 0]
    for a in range(ty):
        for b in range(tx):
            sub = M[a * TILE_H:(a + 1) * TILE_H, b * TILE_W:(b + 1) * TILE_W].reshape(-1, 2)
            sub = sub[sub[:, 0] != OUTSIDE]
            if not len(sub):
                n[2] += 1
                continue
            xi, yi = sub[:, 0] >> 5, sub[:, 1] >> 5
            x0, y0 = int(xi.min()) - 1, int(yi.min()) - 1
            if stage and int(xi.max()) + 2 - x0 + 1 <= WIN_W and int(yi.max()) + 2 - y0 + 1 <= WIN_H:
                tiles[a, b] = (STAGED, x0, y0, 0)
                n[0] += 1
            else:
                tiles[a, b] = (DIRECT, 0, 0, 0)
                n[1] += 1
    return tiles, np.array(n + [int((M[..., 0] == OUTSIDE).sum())], dtype=np.uint32)


# ---- the resampling: integers ---------------------------------------------------------------------------------------------------------

def unclamped(img, M, K=None):
    """img u8 (B, H, W, C) -> int64 (B, ho, wo, C): (acc + 2^21) >> 22 before the clamp to 0 .. 255; an outside pixel's is not used"""
    K = (_weights() if K is None else K).astype(np.int64)
    B, H, W, C = img.shape
    U, V = M[..., 0].astype(np.int64), M[..., 1].astype(np.int64)
    xi, px, yi, py = U >> 5, U & 31, V >> 5, V & 31
    src = img.astype(np.int64)
    acc = np.zeros((B, *M.shape[:2], C), dtype=np.int64)
    for r in range(4):
        yy = np.clip(yi - 1 + r, 0, H - 1)
        row = np.zeros_like(acc)
        for c in range(4):
            row += K[px, c][None, :, :, None] * src[:, yy, np.clip(xi - 1 + c, 0, W - 1), :]
        acc += K[py, r][None, :, :, None] * row
    return (acc + (1 << 21)) >> 22


def undistort(img, M, K=None):
    """img u8 (B, H, W, C) -> u8 (B, ho, wo, C)"""
    out = np.clip(unclamped(img, M, K), 0, 255)
    out[:, M[..., 0] == OUTSIDE] = 0
    return out.astype(np.uint8)


def clamped(img, M):
    """how many values of the inside pixels the clamp raised to 0, and how many it lowered to 255"""
    v = unclamped(img, M)[:, M[..., 0] != OUTSIDE]
    return int((v < 0).sum()), int((v > 255).sum())


# ---- the cases the GPU test and tools/host_check.py share -------------------------------------------------------------------------------

# (B, H, W, C, ho, wo): one pixel (every tap clamps); less than a tile; exactly one tile with both channel counts; one past a tile on
# both axes, a batch of three; several tiles with both channel counts; an output camera of another size
SHAPES = ((1, 1, 1, 1, 1, 1), (1, 7, 9, 3, 7, 9), (1, 8, 32, 1, 8, 32), (1, 8, 32, 3, 8, 32), (3, 9, 33, 1, 9, 33),
          (1, 40, 100, 1, 40, 100), (1, 40, 100, 3, 40, 100), (2, 40, 100, 3, 24, 50))
BARREL, PINCUSHION = (-0.3, 0.1, 1e-3, 1e-3, 0.0), (0.25, 0.05, -1e-3, 5e-4, 0.0)
# name -> (dist, focal_scale, the output principal point's shift in units of the output size)
RIGS = {"identity": ((0.0,) * 5, 1.0, 0.0), "barrel": (BARREL, 1.0, 0.0), "pincushion": (PINCUSHION, 1.0, 0.0),
        "zoom_out": (BARREL, 0.5, 0.0), "aside": (BARREL, 1.0, 0.5)}
PATTERNS = ("noise", "white", "ramp")


def cameras(shape, rig):
    """(src, dst) of a shape under a rig: fx = 0.6 max(W, H) (a field of 80 degrees along the longer side), non-dyadic principal
    points; an output of another size keeps the field"""
    B, H, W, C, ho, wo = shape
    dist, scale, aside = RIGS[rig]
    f = 0.6 * max(W, H)
    src = (W, H, f, 1.03 * f, (W - 1) / 2 + 0.37, (H - 1) / 2 - 0.19, dist)
    g = f * scale * max(wo, ho) / max(W, H)
    dst = (wo, ho, g, 1.03 * g, (wo - 1) / 2 + 0.37 * (1 if (ho, wo) == (H, W) else 0.27) + aside * wo,
           (ho - 1) / 2 - 0.19 + aside * ho, (0.0,) * 5)
    return src, dst


def image(shape, pattern, seed=1):
    B, H, W, C = shape[:4]
    if pattern == "noise":
        return np.random.default_rng(seed + 7 * H + W + C).integers(0, 256, size=(B, H, W, C), dtype=np.uint8)
    if pattern == "white":
        return np.full((B, H, W, C), 255, dtype=np.uint8)
    if pattern == "ramp":
        b, i, j, c = np.meshgrid(np.arange(B), np.arange(H), np.arange(W), np.arange(C), indexing="ij")
        return ((5 * j + 3 * i + 40 * c + 17 * b) % 256).astype(np.uint8)
    raise ValueError(pattern)


def cases(shape):
    return [(rig, pattern) for rig in RIGS for pattern in PATTERNS]


@functools.lru_cache(maxsize=None)
def _tables(shape, rig):
    src, dst = cameras(shape, rig)
    M = map_table(src, dst)
    return (M,) + tile_table(M)


def tables(shape, rig):
    """(M, tiles, counts) of a shape under a rig"""
    return tuple(a.copy() for a in _tables(shape, rig))


@functools.lru_cache(maxsize=None)
def _want(shape, rig, pattern):
    return undistort(image(shape, pattern), _tables(shape, rig)[0])


def want(shape, rig, pattern):
    return _want(shape, rig, pattern).copy()
