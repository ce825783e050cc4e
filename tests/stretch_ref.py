"""numpy restatement of the per-image range normalisation of depth codes (codon_amd/csrc/stretch.hip, codon_amd.upsample.code_range
/ stretch_codes / unstretch_codes) and the inputs its tests share -- TEST INFRASTRUCTURE.  Integers only: the
kernels are held to these bits, no tolerance.

A plane of codes on the grid 0 .. top, 0 a hole; T = top - 1.  Its range (lo, hi): the smallest non-zero and the largest code,
(0, 0) without a valid code.  With n = hi - lo, in 64-bit integer division:
    stretch    0 -> 0;  c -> 1 + (2 k T + n) // (2 n), k = clamp(c, lo, hi) - lo;  n == 0: c -> top
    unstretch  o -> lo + (2 (clamp(o, 1, top) - 1) n + T) // (2 T)
A range that is not 1 <= lo <= hi <= top, (0, 0) above all, makes both the identity."""
import functools

import numpy as np

# (h, w): one code, less than a run of 8, odd sizes, runs with a tail, less than one run per lane of code_range's 1024-lane
# workgroup (64 x 64 = 4096 < 8192), and 67 x 131 = 8777 codes, just above one run per lane (and an odd count: the second image
# of a batch starts off every vector boundary)
PLANES = [(1, 1), (1, 7), (3, 5), (17, 33), (64, 64), (67, 131)]
BATCHES = (1, 3)
SHAPES = [(B, h, w) for B in BATCHES for h, w in PLANES]
PATTERNS = ("holes", "one", "constant", "full", "top2", "tails", "random")
# (name, dtype of the codes, top)
FORMATS = [("u8", np.uint8, 255), ("u16", np.uint16, 65535), ("u16_10000", np.uint16, 10000)]

# the refusals of the three C entries: (what differs from a good call of u16 codes on a 5 x 7 plane, a piece of the message);
# "top" is not an argument of codon_code_range and is left out there
REFUSALS = [({"src": None}, "null pointer"), ({"lo_hi": None}, "null pointer"), ({"out": None}, "null pointer"),
            ({"bits": 12}, "code_bits 12 "), ({"bits": 0}, "code_bits 0 "), ({"B": 0}, "batch 0 "), ({"B": 65536}, "batch 65536 "),
            ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"), ({"h": 16385}, "a 16385x7 plane"),
            ({"w": 16385}, "a 5x16385 plane"), ({"top": 1}, "top 1 "), ({"top": 65536}, "top 65536 "),
            ({"bits": 8, "top": 1000}, "top 1000 "), ({"src": "odd"}, "unaligned"), ({"lo_hi": "odd"}, "unaligned")]


def code_range(c):
    """(lo, hi) of one plane"""
    c = np.asarray(c)
    v = c[c != 0]
    return (int(v.min()), int(v.max())) if v.size else (0, 0)


def ranges(c):
    """(B, 2) int32 of a (B, h, w) batch"""
    return np.asarray([code_range(p) for p in np.asarray(c)], dtype=np.int32).reshape(-1, 2)


def _ok(lo, hi, top):
    return 1 <= lo <= hi <= top


def stretch(c, lo, hi, top):
    """one plane (any shape) with the range (lo, hi), in the plane's dtype"""
    c = np.asarray(c)
    if not _ok(lo, hi, top):
        return c.copy()
    v = c.astype(np.int64)
    n, T = hi - lo, top - 1
    k = np.clip(v, lo, hi) - lo
    s = 1 + (2 * k * T + n) // (2 * n) if n else np.full_like(v, top)
    out = np.where(v == 0, 0, s)
    assert out.min(initial=0) >= 0 and out.max(initial=0) <= top
    return out.astype(c.dtype)


def unstretch(o, lo, hi, top):
    o = np.asarray(o)
    if not _ok(lo, hi, top):
        return o.copy()
    v = np.clip(o.astype(np.int64), 1, top)
    n, T = hi - lo, top - 1
    out = lo + (2 * (v - 1) * n + T) // (2 * T)
    assert out.min(initial=lo) >= lo and out.max(initial=lo) <= hi
    return out.astype(o.dtype)


def stretch_batch(c, top, lo_hi=None):
    """(B, h, w) -> (stretched, (B, 2) ranges); lo_hi None: every plane by its own range"""
    c = np.asarray(c)
    lo_hi = ranges(c) if lo_hi is None else np.asarray(lo_hi, dtype=np.int32).reshape(-1, 2)
    return np.stack([stretch(p, int(lo), int(hi), top) for p, (lo, hi) in zip(c, lo_hi)]), lo_hi


def unstretch_batch(o, lo_hi, top):
    return np.stack([unstretch(p, int(lo), int(hi), top) for p, (lo, hi) in zip(np.asarray(o), np.asarray(lo_hi).reshape(-1, 2))])


# ---- the shared inputs --------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(shape, pattern, top, seed):
    B, h, w = shape
    rng = np.random.default_rng(seed + 7 * B + 31 * h + w)
    c = np.zeros(shape, dtype=np.int64)
    for b in range(B):                                             # a different range per image
        lo = 1 + (top // 9) * (b + 1) % (top - 1)
        hi = min(top, lo + max(2, top // (3 + 2 * b)))
        p = c[b].reshape(-1)
        if pattern == "holes":
            pass
        elif pattern == "one":
            p[(p.size * (b + 1)) // (B + 1)] = lo
        elif pattern == "constant":
            p[:] = hi
        elif pattern == "full":                                    # range (1, top): the stretch must be the identity
            p[:] = rng.integers(1, top + 1, size=p.size)
            p[0], p[-1] = 1, top
            if p.size == 1:
                p[0] = top
        elif pattern == "top2":                                    # a range of two codes at the top of the grid
            p[:] = rng.integers(top - 1, top + 1, size=p.size)
            p[0], p[-1] = top, top - 1
        elif pattern == "tails":                                   # the maximum in the first element, the minimum in the last
            p[:] = rng.integers(lo + 1, hi, size=p.size)
            p[1::3] = 0
            p[0], p[-1] = hi, lo
        elif pattern == "random":
            p[:] = rng.integers(lo, hi + 1, size=p.size)
            p[rng.random(p.size) < 0.3] = 0
        else:
            raise ValueError(pattern)
    c.setflags(write=False)
    return c


def case(shape, pattern, top=255, seed=1):
    """(B, h, w) codes of uint8 (top 255) or uint16, read-only and shared: copy before writing."""
    out = _case(tuple(shape), pattern, int(top), seed).astype(np.uint8 if top == 255 else np.uint16)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _want(shape, pattern, top, seed):
    s, r = stretch_batch(case(shape, pattern, top, seed), top)
    s.setflags(write=False)
    r.setflags(write=False)
    return s, r


def want(shape, pattern, top=255, seed=1):
    """(stretched codes, (B, 2) ranges) of case(...), computed once"""
    return _want(tuple(shape), pattern, int(top), seed)
