"""numpy restatement of the pull-push hole filler (codon_amd/csrc/fill_holes.hip, codon_amd.upsample.fill_holes) and
the inputs its tests share -- TEST INFRASTRUCTURE.  Integers only: the kernels are held to these bits, no tolerance.

A plane of codes, 0 a hole.  Level 0 is the plane, level k+1 has ceil(h_k/2) x ceil(w_k/2) cells, the top level K is the first of
1 x 1.  Pull: a cell is (2 S + n) // (2 n) over its n valid children inside level k (S their sum), a hole when n = 0.  Push from
the top: a valid cell keeps its value, a hole at (y, x) takes (9 F(py,px) + 3 F(py,qx) + 3 F(qy,px) + F(qy,qx) + 8) >> 4 of the
filled level above, py = y >> 1, qy = clamp(py + (+1 if y odd else -1), 0, h_{k+1} - 1), px and qx likewise."""
import functools

import numpy as np

SHAPES = [(1, 1, 1), (1, 5, 7), (3, 9, 13), (2, 64, 64), (1, 65, 67), (1, 70, 200)]
PATTERNS = ("none", "all", "one", "cross", "border", "levels")
MAXIMA = (255, 10000, 65535)
# (name, dtype of the codes, depth_max, fp32 on the grid?)
FORMATS = [("u8", np.uint8, 255, False), ("u16", np.uint16, 65535, False), ("u16_10000", np.uint16, 10000, False),
           ("f32", np.uint16, 10000, True)]


# codon_fill_holes' refusals: (what differs from a good call of u16 codes on a 5 x 7 plane, a piece of the message).  fmt 0 / 1 / 2:
# u8 / u16 / fp32 on the grid; out "src": the input's own buffer; ws_bytes "short": one byte less than needed
REFUSALS = [({"src": None}, "null pointer"), ({"out": None}, "null pointer"), ({"ws": None}, "null pointer"),
            ({"fmt": 2, "tab": None}, "null pointer"), ({"fmt": 3}, "fmt 3 "), ({"fmt": -1}, "fmt -1 "),
            ({"B": 0}, "batch 0 "), ({"B": -2}, "batch -2 "), ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"),
            ({"h": 4097}, "a 4097x7 plane"), ({"w": 4097}, "a 5x4097 plane"), ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "),
            ({"fmt": 0, "top": 1000}, "top 1000 "), ({"out": "src"}, "same buffer"), ({"ws_bytes": "short"}, "too small")]


def levels(h, w):
    """[(h_0, w_0), ..., (h_K, w_K)]"""
    out = [(h, w)]
    while out[-1] != (1, 1):
        out.append(((out[-1][0] + 1) // 2, (out[-1][1] + 1) // 2))
    return out


def workspace_cells(h, w):
    return sum(a * b for a, b in levels(h, w)[1:])


def pull(v):
    """V_{k+1} of V_k (int64, 0 a hole)"""
    h, w = v.shape
    p = np.zeros((2 * ((h + 1) // 2), 2 * ((w + 1) // 2)), dtype=np.int64)
    p[:h, :w] = v                                   # a cell outside the level is no child: it adds to neither n nor S
    q = p.reshape(p.shape[0] // 2, 2, p.shape[1] // 2, 2)
    n = (q != 0).sum(axis=(1, 3))
    s = q.sum(axis=(1, 3))
    return np.where(n > 0, (2 * s + n) // np.maximum(2 * n, 1), 0)


def push(v, f_up):
    """F_k of V_k and F_{k+1}"""
    h, w = v.shape
    hu, wu = f_up.shape
    y, x = np.arange(h), np.arange(w)
    py, px = y >> 1, x >> 1
    qy = np.clip(py + np.where(y & 1, 1, -1), 0, hu - 1)
    qx = np.clip(px + np.where(x & 1, 1, -1), 0, wu - 1)
    mix = (9 * f_up[np.ix_(py, px)] + 3 * f_up[np.ix_(py, qx)] + 3 * f_up[np.ix_(qy, px)] + f_up[np.ix_(qy, qx)] + 8) >> 4
    assert mix.max(initial=0) < 1 << 31
    return np.where(v != 0, v, mix)


def fill_plane(c, with_levels=False):
    """F_0 of one (h, w) plane of codes, in the plane's dtype.  with_levels: (F_0, anc) with anc (h, w) int: 0 at a valid pixel,
    at a hole the pyramid level of its nearest valid ancestor (the smallest k with V_k(y >> k, x >> k) valid), K + 1 when the
    plane has no valid pixel."""
    c = np.asarray(c)
    v = [c.astype(np.int64)]
    while v[-1].shape != (1, 1):
        v.append(pull(v[-1]))
    K = len(v) - 1
    assert [a.shape for a in v] == levels(*c.shape)
    f = v[K]
    for k in range(K - 1, -1, -1):
        f = push(v[k], f)
    out = f.astype(c.dtype)
    assert np.array_equal(out, f)
    if not with_levels:
        return out
    yy, xx = np.mgrid[0:c.shape[0], 0:c.shape[1]]
    anc = np.full(c.shape, K + 1, dtype=np.int64)
    for k in range(K, -1, -1):
        anc = np.where(v[k][yy >> k, xx >> k] != 0, k, anc)
    return out, anc


def fill(c):
    """fill_plane over a (B, h, w) batch"""
    return np.stack([fill_plane(p) for p in np.asarray(c)])


def check_consequences(c, f, top):
    """What the definition promises of the filled plane f of c (one plane), asserted."""
    c, f = np.asarray(c), np.asarray(f)
    valid = c != 0
    assert f.shape == c.shape and f.dtype == c.dtype
    assert np.array_equal(f[valid], c[valid])                      # valid pixels come back bit-identical
    if valid.all() or not valid.any():
        assert np.array_equal(f, c)                                # nothing to fill, or nothing to fill from
    if valid.any():
        assert f.min() >= 1 and f.max() <= c[valid].max() <= top   # never a hole, never above the largest valid code
    if valid.sum() == 1:
        assert (f == c[valid][0]).all()                            # one valid pixel fills the plane


def table(depth_max):
    """code_table's table: float32(float64(c) / depth_max) for every code (upsample.u8_lut / lut16)"""
    return (np.arange(65536 if depth_max != 255 else 256, dtype=np.float64) / depth_max).astype(np.float32)


def to_grid(c, depth_max):
    """codes -> fp32 on the code grid (a hole is +0.0)"""
    return table(depth_max)[np.asarray(c).astype(np.int64)]


def from_grid(v, depth_max):
    return np.rint(np.asarray(v, dtype=np.float32) * np.float32(depth_max)).astype(np.int64)


# ---- the shared inputs --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(shape, pattern, top, seed):
    B, h, w = shape
    rng = np.random.default_rng(seed)
    lo = max(1, top // 8)
    c = rng.integers(lo, top + 1, size=shape).astype(np.int64)
    c[:, ::3, ::2] = top                                           # the maximum itself is there
    if pattern == "none":
        pass
    elif pattern == "all":
        c[:] = 0
    elif pattern == "one":
        keep = c[:, h // 2, w - 1 - w // 3].copy()
        c[:] = 0
        c[:, h // 2, w - 1 - w // 3] = keep
    elif pattern == "cross":
        c[:, h // 2, :] = 0
        c[:, :, w // 3] = 0
    elif pattern == "border":
        c[:, 0, :] = c[:, -1, :] = 0
        c[:, :, 0] = c[:, :, -1] = 0
        c[:, :min(3, h), :min(3, w)] = 0
        c[:, max(h - 2, 0):, max(w - 4, 0):] = 0
    elif pattern == "levels":
        c[rng.random(shape) < 0.06] = 0
        k = 1
        while 2 ** k < max(h, w):
            c[:, 2 ** k:2 ** (k + 1), 2 ** k:2 ** (k + 1)] = 0
            k += 1
        if (h, w) == (70, 200):
            c[:, :, 128:] = 0
    else:
        raise ValueError(pattern)
    c.setflags(write=False)
    return c


def case(shape, pattern, top=255, seed=1):
    """(B, h, w) codes of uint8 (top 255) or uint16, read-only and shared: copy before writing."""
    c = _case(tuple(shape), pattern, int(top), seed)
    out = c.astype(np.uint8 if top == 255 else np.uint16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(shape, pattern, top, seed):
    out = fill(case(shape, pattern, top, seed))
    out.setflags(write=False)
    return out


def want(shape, pattern, top=255, seed=1):
    """fill(case(...)), computed once"""
    return _want(tuple(shape), pattern, int(top), seed)
