"""numpy restatement of the guidance-aware (joint) pull-push hole filler (codon_amd/csrc/fill_guided.hip,
codon_amd.upsample.fill_holes_guided) and the inputs its tests share -- TEST INFRASTRUCTURE.  Integers only: the
kernels are held to these bits, no tolerance.  The depth pyramid is the plain filler's (tests/fill_ref.py: levels, pull).

Codes c (h x w, 0 a hole), guidance g (u8, the top-left h s x w s of it), scale s, range table T (256 entries in 1 .. 256).
Guidance pyramid: G_0 the s x s box mean, G_{k+1} the mean over the children inside level k, halves rounded up.  Beside V rides
the attached guidance A: A_0 = G_0 at valid pixels, A_{k+1} the mean of A_k over the valid children that entered V_{k+1}.  Push: a
hole at (y, x) of level k weighs the plain filler's four parents p by w_p = B_p T[|G_k(y, x) - A^_{k+1}(p)|], B = 9, 3, 3, 1, with
A^ = A where V is valid and G where it is a hole, and takes (2 sum w_p F_{k+1}(p) + sum w_p) // (2 sum w_p)."""
import functools

import numpy as np

from tests import fill_ref as F

SCALES = (4, 8, 16)
SIGMA = 10.0
# the scale each fill_ref shape is run at where a test does not cross shapes with scales
SHAPE_SCALE = {(1, 1, 1): 4, (1, 5, 7): 4, (3, 9, 13): 8, (2, 64, 64): 4, (1, 65, 67): 16, (1, 70, 200): 4}
GUIDES = ("random", "constant", "scene")
# 2 * 4096 * 65535 + 4096: the largest numerator of a filled value (sum w_p <= 16 * 256)
NUMERATOR_MAX = 2 * 16 * 256 * 65535 + 16 * 256
assert NUMERATOR_MAX < 1 << 31

# codon_fill_holes_guided's refusals: (what differs from a good call of u16 codes on a 5 x 7 plane at x4, a piece of the message)
REFUSALS = [({"src": None}, "null pointer"), ({"out": None}, "null pointer"), ({"ws": None}, "null pointer"),
            ({"guide": None}, "null pointer"), ({"tab": None}, "null pointer"), ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "),
            ({"B": 0}, "batch 0 "), ({"B": 65536}, "batch 65536 "), ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"),
            ({"h": 4097}, "a 4097x7 plane"), ({"w": 4097}, "a 5x4097 plane"), ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "),
            ({"fmt": 0, "top": 1000}, "top 1000 "), ({"scale": 2}, "scale 2 "), ({"scale": 32}, "scale 32 "),
            ({"row_bytes": 27}, "guide rows of 27 bytes"), ({"B": 2, "image_bytes": 20 * 28 - 1}, "guide images 559 bytes apart"),
            ({"out": "src"}, "same buffer"), ({"ws_bytes": "short"}, "too small")]


def range_table(sigma=SIGMA):
    """T[d] = max(1, rint(256 exp(-d^2 / (2 sigma^2)))), float64, as (256,) uint16"""
    d = np.arange(256, dtype=np.float64)
    return np.maximum(1.0, np.rint(256.0 * np.exp(-d * d / (2.0 * float(sigma) ** 2)))).astype(np.uint16)


def workspace_bytes(h, w):
    """One image: V (u16), A and G (u8) of levels 1 .. K, and G_0 (u8)"""
    return 4 * F.workspace_cells(h, w) + h * w


def guide_base(g, h, w, s):
    """G_0: the box mean of the top-left (h s, w s) of g, half rounded up"""
    g = np.asarray(g)
    assert g.dtype == np.uint8 and g.shape[0] >= h * s and g.shape[1] >= w * s
    tot = g[:h * s, :w * s].astype(np.int64).reshape(h, s, w, s).sum(axis=(1, 3))
    return (2 * tot + s * s) // (2 * s * s)


def _blocks(a):
    h, w = a.shape
    p = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), dtype=np.int64)
    p[:h, :w] = a
    return p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2)


def pull_guide(G):
    """G_{k+1} of G_k: the mean over the children inside level k"""
    n = _blocks(np.ones_like(G)).sum(axis=(1, 3))
    return (2 * _blocks(G).sum(axis=(1, 3)) + n) // (2 * n)


def pull_attached(V, A):
    """A_{k+1} of V_k and A_k: the mean of A_k over the valid children (0, unused, where there is none)"""
    valid = (V != 0).astype(np.int64)
    n = _blocks(valid).sum(axis=(1, 3))
    return np.where(n > 0, (2 * _blocks(A * valid).sum(axis=(1, 3)) + n) // np.maximum(2 * n, 1), 0)


def push(V, G, F_up, V_up, A_up, G_up, T):
    """F_k of V_k, G_k and level k + 1"""
    h, w = V.shape
    hu, wu = F_up.shape
    y, x = np.arange(h), np.arange(w)
    py, px = y >> 1, x >> 1
    qy = np.clip(py + np.where(y & 1, 1, -1), 0, hu - 1)
    qx = np.clip(px + np.where(x & 1, 1, -1), 0, wu - 1)
    hat = np.where(V_up != 0, A_up, G_up)
    T = np.asarray(T).astype(np.int64)
    num = np.zeros((h, w), dtype=np.int64)
    den = np.zeros((h, w), dtype=np.int64)
    for base, iy, ix in ((9, py, px), (3, py, qx), (3, qy, px), (1, qy, qx)):
        wgt = base * T[np.abs(G - hat[np.ix_(iy, ix)])]
        num += wgt * F_up[np.ix_(iy, ix)]
        den += wgt
    assert den.min(initial=16) >= 16 and (2 * num + den).max(initial=0) <= NUMERATOR_MAX < 1 << 31
    return np.where(V != 0, V, (2 * num + den) // (2 * den))


def fill_plane(c, g, s, T):
    """F_0 of one (h, w) plane of codes and its guidance, in the plane's dtype"""
    c = np.asarray(c)
    h, w = c.shape
    T = np.asarray(T)
    assert T.shape == (256,) and T.min() >= 1 and T.max() <= 256 and s in SCALES
    V, G = [c.astype(np.int64)], [guide_base(g, h, w, s)]
    A = [np.where(V[0] != 0, G[0], 0)]
    while V[-1].shape != (1, 1):
        A.append(pull_attached(V[-1], A[-1]))
        V.append(F.pull(V[-1]))
        G.append(pull_guide(G[-1]))
    K = len(V) - 1
    assert [a.shape for a in V] == [a.shape for a in G] == [a.shape for a in A] == F.levels(h, w)
    f = V[K]
    for k in range(K - 1, -1, -1):
        f = push(V[k], G[k], f, V[k + 1], A[k + 1], G[k + 1], T)
    out = f.astype(c.dtype)
    assert np.array_equal(out, f)
    return out


def fill(c, g, s, T):
    """fill_plane over a (B, h, w) batch with (B, H, W) guidance"""
    return np.stack([fill_plane(p, q, s, T) for p, q in zip(np.asarray(c), np.asarray(g))])


# ---- the shared inputs --------------------------------------------------------------------------------------------------------

def edge_of(y, w):
    """the occlusion edge: a pixel is near (foreground) when x < edge_of(y, w), in low-resolution pixels"""
    return 0.45 * w + 0.25 * y


@functools.lru_cache(maxsize=None)
def scene(h, w, s, top, seed=3):
    """(codes, guide, truth) of the occlusion scene: a slanted depth edge, near depth top / 4 and far depth 3 top / 4 with +-2
    codes of noise, guidance 190 / 70 with sigma-4 noise rendered at high resolution from the same edge, holes the six-pixel
    band on the far side of the edge plus 3 % random ones.  codes, truth: (h, w) uint8 (top 255) or uint16; guide (h s, w s)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    edge = edge_of(yy, w)
    near = xx < edge
    truth = np.clip(np.where(near, top // 4, 3 * top // 4) + rng.integers(-2, 3, size=(h, w)), 1, top)
    Y, X = np.mgrid[0:h * s, 0:w * s]
    near_hr = X / s < edge_of(Y / s, w)
    guide = np.clip(np.rint(np.where(near_hr, 190.0, 70.0) + rng.normal(0.0, 4.0, size=near_hr.shape)), 0, 255).astype(np.uint8)
    holes = (~near & (xx < edge + 6)) | (rng.random((h, w)) < 0.03)
    dt = np.uint8 if top == 255 else np.uint16
    codes = np.where(holes, 0, truth).astype(dt)
    truth = truth.astype(dt)
    for a in (codes, guide, truth):
        a.setflags(write=False)
    return codes, guide, truth


def hole_error(filled, codes, truth):
    """mean absolute error over the holes, in codes"""
    holes = np.asarray(codes) == 0
    return float(np.abs(np.asarray(filled).astype(np.int64) - np.asarray(truth).astype(np.int64))[holes].mean())


@functools.lru_cache(maxsize=None)
def guide_case(shape, s, kind, seed=7):
    """(B, h s, w s) uint8 guidance for a fill_ref case: "random", "constant" (113) or "scene" (the occlusion scene's)"""
    B, h, w = shape
    if kind == "random":
        g = np.random.default_rng(seed).integers(0, 256, size=(B, h * s, w * s), dtype=np.uint8)
    elif kind == "constant":
        g = np.full((B, h * s, w * s), 113, dtype=np.uint8)
    elif kind == "scene":
        g = np.stack([scene(h, w, s, 255, seed=3 + b)[1] for b in range(B)])
    else:
        raise ValueError(kind)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _table(table):
    t = np.full(256, int(table[1:]), dtype=np.uint16) if isinstance(table, str) else range_table(table)
    t.setflags(write=False)
    return t


def table_of(table):
    """a float is sigma; "c<n>" the constant table of n"""
    return _table(table)


@functools.lru_cache(maxsize=None)
def want(shape, pattern, top, s, kind, table, seed=1):
    """fill(fill_ref.case(...), guide_case(...)), computed once"""
    out = fill(F.case(shape, pattern, top, seed), guide_case(tuple(shape), s, kind), s, table_of(table))
    out.setflags(write=False)
    return out
