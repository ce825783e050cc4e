"""numpy restatement of the spatial smoothing of sensor depth maps (codon_amd/csrc/smooth.hip, codon_amd.smooth) and
the inputs its tests share -- TEST INFRASTRUCTURE.  Integers only: the kernel is held to these bits, no tolerance.  A DEFINITION of
this project.

Codes c (B, h, w), u8 or u16, 0 a hole.  Two codes are LINKED under clean's rule (tests/clean_ref.linked): both non-zero and at
most tau(min) = A + ((Rq min) >> 16) apart.  The weight table W of (radius R, sigma): (2R+1)^2 entries rint(256 exp(-(dy^2 + dx^2)
/ (2 sigma^2))), all 256 for sigma None; the centre is 256, the table is symmetric under (dy, dx) -> (-dy, -dx), an entry may be 0.
One pass c -> c': a hole stays 0.  For a valid pixel p, S = the window positions q != p inside the plane that are linked to c_p (the
codes of the pass's input); with `pairs`, q stays in S only if its mirror 2p - q is inside the plane and linked to c_p too.
N = 256 c_p + sum_S W_q c_q, D = 256 + sum_S W_q, c'_p = (2N + D) // (2D).  P passes compose; a pixel outside the plane is a hole in
every pass.  Statistics per image, four u32: valid inputs, pixels whose final code differs from the input, valid pixels whose S is
empty in the first pass, the largest |final - input|."""
import functools

import numpy as np

from tests.clean_ref import linked, rel_q16  # noqa: F401  (the one link rule; rel_q16 for the callers)

MAX_SIDE, MAX_RADIUS, MAX_PASSES, MAX_REL = 4096, 4, 3, 65535
STATS = ("valid", "changed", "alone", "max")
DEFAULTS = dict(radius=2, passes=2, sigma=None, tolerance=2, tolerance_rel=0.02, pairs=True)
RQ = rel_q16(0.02)                          # 1311


def weight_table(radius, sigma=None):
    """(2R+1, 2R+1) int32"""
    side = 2 * radius + 1
    if sigma is None:
        return np.full((side, side), 256, dtype=np.int32)
    d = np.arange(-radius, radius + 1, dtype=np.float64)
    return np.rint(256.0 * np.exp(-(d[:, None] ** 2 + d[None, :] ** 2) / (2.0 * float(sigma) ** 2))).astype(np.int32)


def tau(c, A, Rq):
    """The most one pass moves a code c"""
    return A + ((Rq * np.asarray(c, dtype=np.int64)) >> 16)


def one_pass(c, W, A, Rq, pairs):
    """One pass over one plane (int64 (h, w)) -> (c', the mask of the valid pixels whose S is empty)"""
    h, w = c.shape
    R = W.shape[0] // 2
    pad = np.zeros((h + 2 * R, w + 2 * R), dtype=np.int64)   # outside the plane: a hole, linked to nothing
    pad[R:R + h, R:R + w] = c
    N, D, n = 256 * c, np.full((h, w), 256, dtype=np.int64), np.zeros((h, w), dtype=np.int64)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if (dy, dx) == (0, 0):
                continue
            q = pad[R + dy:R + dy + h, R + dx:R + dx + w]
            s = linked(c, q, A, Rq)
            if pairs:
                s = s & linked(c, pad[R - dy:R - dy + h, R - dx:R - dx + w], A, Rq)
            N, D, n = N + int(W[dy + R, dx + R]) * s * q, D + int(W[dy + R, dx + R]) * s, n + s
    assert (2 * N + D).max(initial=0) < 1 << 32
    return np.where(c != 0, (2 * N + D) // (2 * D), 0), (c != 0) & (n == 0)


def smooth_plane(c, radius, passes, sigma, A, Rq, pairs):
    """One plane of codes -> (codes of its dtype, four u32 statistics)"""
    W = weight_table(radius, sigma)
    first = cur = c.astype(np.int64)
    alone = None
    for _ in range(passes):
        cur, lonely = one_pass(cur, W, A, Rq, pairs)
        alone = lonely if alone is None else alone
    d = np.abs(cur - first)
    stats = np.array([(first != 0).sum(), (d != 0).sum(), alone.sum(), d.max(initial=0)], dtype=np.uint32)
    return cur.astype(c.dtype), stats


def smooth(c, radius=2, passes=2, sigma=None, A=2, Rq=RQ, pairs=True):
    """(B, h, w) codes -> (codes, (B, 4) uint32)"""
    rows = [smooth_plane(p, radius, passes, sigma, A, Rq, pairs) for p in c]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


# ---- the seeded scene of the CPU test (DESIGN 12.25's numbers) -----------------------------------------------------------------------

SCENE_SHAPE = (96, 128)
SCENE_NOISE = {255: 3, 10000: 12}


def scene(top, seed=20):
    """(noisy codes with 5 % holes, noiseless codes): a slanted background and a steeper slanted rectangle, the step between them
    far larger than tau"""
    h, w = SCENE_SHAPE
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 60.0 + 0.37 * x + 0.21 * y
    rect = (y > 20) & (y < 70) & (x > 30) & (x < 90)
    v = np.where(rect, 150.0 + 0.9 * (x - 40.0), v) * (top / 255.0)
    g = np.random.default_rng(seed)
    noise = g.uniform(-SCENE_NOISE[top], SCENE_NOISE[top], size=(h, w))
    dt = np.uint8 if top == 255 else np.uint16
    noisy = np.clip(np.rint(v + noise), 1, top).astype(dt)
    noisy[g.random((h, w)) < 0.05] = 0
    return noisy, np.rint(v).astype(dt)


def mae(got, clean):
    """The mean absolute error over the valid pixels of `got`"""
    m = got != 0
    return float(np.abs(got.astype(np.int64) - clean.astype(np.int64))[m].mean())


# ---- the cases the GPU test and the host check share ---------------------------------------------------------------------------------

TILE = 32                                   # SM_TILE of codon_amd/csrc/smooth_tile.h


def fuse_bound(radius):
    """smooth_fuse_bound of codon_amd/csrc/launch_rules.h: the most passes one launch runs"""
    return 3 if radius == 1 else 1


def launches(radius, passes):
    """smooth_launches of codon_amd/csrc/launch_rules.h"""
    k = min(passes, fuse_bound(radius))
    return -(-passes // k)


PLANES = ((1, 1), (1, 7), (9, 1), (3, 3), (TILE, TILE), (TILE - 1, TILE + 1), (TILE + 1, 2 * TILE + 1), (2 * TILE + 3, 67))
RADII, PASSES, SIGMAS = (1, 2, 4), (1, 2, 3), (None, 0.8)
FORMATS = (255, 10000, 65535)               # top: u8; u16 of a data set; u16 with codes of 32768 and more
PATTERNS = ("none", "all", "random", "checker", "top")      # all holes; no holes; 30 % holes; two levels; codes at top
TOLERANCES = ("zero", "default", "top")     # (A, rel) = (0, 0), (2, 0.02), (top, 0)


def tolerance_of(form, top):
    return {"zero": (0, 0), "default": (2, RQ), "top": (top, 0)}[form]


def plane(B, h, w, pattern, top, seed=1):
    """(B, h, w) codes of the dtype of `top`"""
    g = np.random.default_rng([seed, B, h, w, PATTERNS.index(pattern), top])
    dt = np.uint8 if top == 255 else np.uint16
    y, x = np.mgrid[0:h, 0:w]
    if pattern == "none":
        return np.zeros((B, h, w), dtype=dt)
    if pattern == "checker":
        lo = top // 3
        c = np.broadcast_to(np.where((y + x) % 2 == 0, lo, lo + 3), (B, h, w)).astype(dt)
        return np.ascontiguousarray(c)
    if pattern == "top":
        return (top - g.integers(0, 4, size=(B, h, w))).astype(dt)
    # a slanted surface at 0.55 .. 0.95 of top, a nearer block in one corner, noise of a few tau
    base = top * (0.55 + 0.4 * (x / max(w, 1) + 2 * y / max(h, 1)) / 3.0)
    base = np.where((y < h // 2) & (x >= w // 2), 0.2 * top + 0.5 * x, base)
    noise = g.integers(-3 - top // 400, 4 + top // 400, size=(B, h, w))
    c = np.clip(np.rint(base)[None].astype(np.int64) + noise, 1, top).astype(dt)
    if pattern == "random":
        c[g.random((B, h, w)) < 0.3] = 0
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """(B, h, w, radius, passes, sigma, pairs, A, Rq, pattern, top): every plane under every (radius, passes) with the pair rule on
    and off; sigma, the tolerances, the formats, the patterns and the batch in turn"""
    rows, n = [], 0
    for h, w in PLANES:
        for R in RADII:
            for P in PASSES:
                for pairs in (True, False):
                    top = FORMATS[(n // 3) % 3]
                    A, Rq = tolerance_of(TOLERANCES[n % 3], top)
                    rows.append((3 if n % 4 == 1 else 1, h, w, R, P, SIGMAS[(n // 6) % 2], pairs, A, Rq, PATTERNS[n % 5], top))
                    n += 1
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def codes_of(case):
    B, h, w, R, P, sigma, pairs, A, Rq, pattern, top = case
    c = plane(B, h, w, pattern, top)
    c.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def want(case):
    """(codes, (B, 4) uint32) of a case, computed once and shared"""
    B, h, w, R, P, sigma, pairs, A, Rq, pattern, top = case
    out, stats = smooth(codes_of(case), R, P, sigma, A, Rq, pairs)
    out.setflags(write=False), stats.setflags(write=False)
    return out, stats
