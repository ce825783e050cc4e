"""numpy restatement of the temporal filter of a fixed camera's depth sequence (codon_amd/csrc/temporal.hip, codon_amd.temporal;
DESIGN 12.23) and the inputs its tests share -- TEST INFRASTRUCTURE.  Integers only, int64 inside: the kernel is held to these
bits, no tolerance.  A DEFINITION of this project.

Codes c (T, h, w), u8 or u16, 0 a hole, frame order being time.  The window of frame t is s in [max(0, t - Bk), min(T - 1, t + Ah)],
n_w frames, at most 15.  tau(x) = A + ((Rq x) >> 16); u and v are LINKED iff both are non-zero and |u - v| <= tau(min(u, v)) --
clean's rule (tests/clean_ref.py), restated here and compared in tests/test_temporal_cpu.py.  Per pixel p and frame t, v = c_t(p),
every read of c, never of the output (one pass, not idempotent):
1. v != 0: Lk = the window samples linked to v (v among them), n = |Lk| >= 1.  n >= min(M, n_w): out = (2 sum Lk + n) // (2 n), the
   mean rounded half up.  Otherwise p is REJECTED and goes on with 2 over all non-zero samples, v included.
2. v == 0, or rejected: F == 0: out = 0.  Otherwise S = the non-zero window samples, k = |S|; k < F: out = 0; else m = the lower
   median of S, the element of rank (k - 1) >> 1 in sorted order, Lm = the samples linked to m, and out = the rounded mean of Lm if
   |Lm| >= F, else 0.  F is not clamped by n_w.
Statistics per frame, four u32: valid (input != 0), rejected, filled (output != 0 where the input was 0 or rejected), changed (input
!= 0, not rejected, output != input)."""
import functools

import numpy as np

MAX_FRAMES, MAX_SIDE, MAX_WINDOW, MAX_REL = 4096, 4096, 15, 65535
STATS = ("valid", "rejected", "filled", "changed")
DEFAULTS = dict(window=5, causal=False, tolerance=2, tolerance_rel=0.02, min_count=2, min_fill=2)     # the last four: untuned


def rel_q16(rel):
    """Rq of a relative tolerance in [0, 1)"""
    q = int(np.rint(65536.0 * float(rel)))
    assert 0 <= q <= MAX_REL
    return q


def linked(a, b, A, Rq):
    """Elementwise: a and b (int64 arrays of codes) are linked"""
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    return (lo != 0) & (hi - lo <= A + ((Rq * lo) >> 16))


def rint_mean(total, n):
    """(2 total + n) // (2 n) where n > 0, else 0"""
    return np.where(n > 0, (2 * total + n) // np.maximum(2 * n, 1), 0)


def lower_median(S):
    """Per pixel of S (n_w, ...) int64: the element of rank (k - 1) >> 1 among the k non-zero samples in sorted order; 0 where k = 0"""
    k = (S != 0).sum(axis=0)
    srt = np.sort(np.where(S != 0, S, np.iinfo(np.int64).max), axis=0)          # the holes behind the samples
    m = np.take_along_axis(srt, (np.maximum(k - 1, 0) >> 1)[None], axis=0)[0]
    return np.where(k > 0, m, 0), k


def window_of(t, T, back, ahead):
    return max(0, t - back), min(T - 1, t + ahead)


def temporal(c, back, ahead, tolerance, tolerance_rel_q16, min_count, min_fill, details=False):
    """(out (T, h, w) in c's dtype, stats (T, 4) uint32) of one sequence of unsigned codes; details: and the rejected mask"""
    c = np.asarray(c)
    assert c.ndim == 3 and c.dtype in (np.uint8, np.uint16)
    Bk, Ah, A, Rq, M, F = int(back), int(ahead), int(tolerance), int(tolerance_rel_q16), int(min_count), int(min_fill)
    T = c.shape[0]
    assert 1 <= T <= MAX_FRAMES and Bk >= 0 and Ah >= 0 and Bk + Ah < MAX_WINDOW and c.size < 1 << 31
    assert 0 <= A <= 65535 and 0 <= Rq <= MAX_REL and 1 <= M <= MAX_WINDOW and 0 <= F <= MAX_WINDOW
    x = c.astype(np.int64)
    out = np.zeros_like(x)
    rej_all = np.zeros(x.shape, dtype=bool)
    stats = np.zeros((T, 4), dtype=np.uint32)
    for t in range(T):
        lo, hi = window_of(t, T, Bk, Ah)
        S, v = x[lo:hi + 1], x[t]
        nw = hi - lo + 1
        Lk = linked(v[None], S, A, Rq)
        n = Lk.sum(axis=0)
        kept = (v != 0) & (n >= min(M, nw))
        rejected = (v != 0) & ~kept
        o = np.where(kept, rint_mean((S * Lk).sum(axis=0), n), 0)
        if F > 0:
            m, k = lower_median(S)
            Lm = linked(m[None], S, A, Rq)
            nm = Lm.sum(axis=0)
            o = np.where(~kept & (k >= F) & (nm >= F), rint_mean((S * Lm).sum(axis=0), nm), o)
        out[t], rej_all[t] = o, rejected
        stats[t] = ((v != 0).sum(), rejected.sum(), (~kept & (o != 0)).sum(), (kept & (o != v)).sum())
    out = out.astype(c.dtype)
    return (out, stats, rej_all) if details else (out, stats)


# ---- the launch rules the tests place their sizes around (codon_amd/csrc/launch_rules.h; compared with the library's answer) ------

TILE, PER = 1024, 4                         # TP_TILE, TP_PER of codon_amd/csrc/temporal_tile.h
WORKGROUPS, MIN_CHUNK = 1024, 8


def chunk_frames(T, h, w, back, ahead):
    groups = -(-h * w // TILE)
    want = -(-WORKGROUPS // groups)
    return min(max(-(-T // want), 2 * (back + ahead), MIN_CHUNK), T)


# ---- the scene: a static rig, a rectangle that moves, range noise, flicker, spikes, a band that never measures ----------------------

SCENE_T, SCENE_H, SCENE_W, SCENE_TOP = 16, 40, 100, 10000
RECT_ROWS, RECT_W, RECT_X0, RECT_STEP = (8, 32), 40, 10, 4      # rows [8, 32), 40 columns from rect_x(t): 24 x 40 at 1000
REST = 2                                    # the rectangle stands still in the first REST + 1 frames and in the last
BAND_ROWS = (34, 37)                        # three rows that are holes in every frame
N_FLICKER, N_SPIKES = 600, 60               # pixels that are a hole in one frame, and that hold a random far code in one frame
SCENE_SEED = 1
SCENE_TOLERANCE = {255: 1, 10000: 8, 65535: 52}             # A per top: 8 codes of 10000, scaled (clean_ref's)
NEAR_HI, FAR_LO = 1003, 2997                # the two surfaces' bands at top 10000: codes strictly between these are on neither


def _scaled(c, top):
    if top == SCENE_TOP:
        return c
    return np.where(c != 0, np.maximum(np.rint(c * (top / SCENE_TOP)).astype(np.int64), 1), 0)


def rect_x(t):
    """The rectangle's first column in frame t: at rest in frames 0 .. 2, four columns further in each of frames 3 .. 13, at rest
    again in frames 13 .. 15 -- a surface seen in ONE frame of a window is a spike to the filter, at the sequence's ends too"""
    return RECT_X0 + RECT_STEP * min(max(t - REST, 0), SCENE_T - 1 - 2 * REST)


def rect_mask(t):
    m = np.zeros((SCENE_H, SCENE_W), dtype=bool)
    m[RECT_ROWS[0]:RECT_ROWS[1], rect_x(t):rect_x(t) + RECT_W] = True
    return m


def path_mask(margin=1):
    """Every pixel the rectangle covers in some frame, and `margin` pixels around"""
    m = np.zeros((SCENE_H, SCENE_W), dtype=bool)
    m[RECT_ROWS[0] - margin:RECT_ROWS[1] + margin, rect_x(0) - margin:rect_x(SCENE_T - 1) + RECT_W + margin] = True
    return m


def scene_truth(top=SCENE_TOP):
    """(16, 40, 100) int64: the noiseless frames on the grid of `top`, the band included (no holes)"""
    far = np.broadcast_to(3000 + 2 * np.arange(SCENE_W)[None, :], (SCENE_H, SCENE_W))
    return _scaled(np.stack([np.where(rect_mask(t), 1000, far) for t in range(SCENE_T)]).astype(np.int64), top)


@functools.lru_cache(maxsize=None)
def scene(top=SCENE_TOP, seed=SCENE_SEED):
    """(codes (16, 40, 100), flicker mask, spike mask) of the scene on the grid of `top`: a background at 3000 + 2 column and a
    24 x 40 rectangle at 1000 that moves four columns per frame in frames 3 .. 13 (rect_x), both with fresh +- 3 codes of noise in
    every frame; 600 pixels outside the band that are a hole in one frame each (flicker) and 60 others that hold a random code in
    5000 .. 9000 in one frame each (spikes): one event per pixel; rows 34 .. 36 holes in every frame.  Other tops: the codes of top
    10000, scaled and rounded"""
    g = np.random.default_rng([seed, 12, 23])
    c = scene_truth(SCENE_TOP) + g.integers(-3, 4, size=(SCENE_T, SCENE_H, SCENE_W))
    free = np.ones((SCENE_H, SCENE_W), dtype=bool)
    free[BAND_ROWS[0]:BAND_ROWS[1]] = False
    where = g.permutation(np.flatnonzero(free))[:N_FLICKER + N_SPIKES]
    when = g.integers(0, SCENE_T, size=where.size)
    flicker = np.zeros(c.shape, dtype=bool)
    spikes = np.zeros(c.shape, dtype=bool)
    flicker.reshape(SCENE_T, -1)[when[:N_FLICKER], where[:N_FLICKER]] = True
    spikes.reshape(SCENE_T, -1)[when[N_FLICKER:], where[N_FLICKER:]] = True
    c[spikes] = g.integers(5000, 9001, size=N_SPIKES)
    c[flicker] = 0
    c[:, BAND_ROWS[0]:BAND_ROWS[1]] = 0
    c = _scaled(c, top)
    out = c.astype(np.uint8 if top == 255 else np.uint16)
    assert np.array_equal(out, c)
    for a in (out, flicker, spikes):
        a.setflags(write=False)
    return out, flicker, spikes


# ---- the shared cases of the GPU test and of the host-side check ----------------------------------------------------------------------

# (h, w): one pixel; a single row; odd sizes; 17 x 17; the scene's size (four pixel groups, the last one partial, whole quads);
# a width one more than a multiple of the four pixels a thread owns (a partial last quad); 4 x 8, whole quads on a small plane
PLANES = ((1, 1), (1, 37), (5, 7), (17, 17), (40, 100), (9, 29), (4, 8))
BIG_PLANE = (40, 100)                       # runs the short sequences alone
FORMATS = (("u8", 255), ("u16", 65535), ("u16_10000", 10000))
WINDOWS = ((0, 0), (1, 1), (7, 7), (14, 0), (0, 14), (2, 5), (2, 2))         # (Bk, Ah); (2, 2): the default, five window registers
# (M, F, A or None for the top's own, Rq or None for the default's)
PARAMS = ((1, 0, None, None), (2, 2, None, None), (15, 15, None, None), (2, 0, None, None), (1, 3, None, None),
          (2, 2, 0, None), (2, 2, None, 0))
PATTERNS = ("random", "all", "none", "scene", "high", "single")
SHORT = (1, 2, 3, 15, 16, 17)


def lengths(plane, window):
    """The T of a plane under a window: the short ones, and around the chunk length L -- L - 1, L, L + 1 and two chunks + 1"""
    if plane == BIG_PLANE:
        return (1, 3, 16, 17)
    L = chunk_frames(MAX_FRAMES, *plane, *window)
    return tuple(sorted(set(SHORT + (L - 1, L, L + 1, 2 * L + 1))))


def cases():
    """[(T, h, w, Bk, Ah, M, F, A, Rq, pattern, top)]: every plane under every window at every length, the parameters, patterns and
    formats in turn -- but `high` on the full u16 grid always, and the scene at its own length on its own plane"""
    rows = []
    for pi, plane in enumerate(PLANES):
        for wi, window in enumerate(WINDOWS):
            for ti, T in enumerate(lengths(plane, window)):
                M, F, A, Rq = PARAMS[(pi + wi + ti) % len(PARAMS)]
                pattern = PATTERNS[(pi + 2 * wi + 3 * ti) % len(PATTERNS)]
                top = 65535 if pattern == "high" else FORMATS[(pi + wi + 2 * ti) % 3][1]
                rows.append((T, *plane, *window, M, F, SCENE_TOLERANCE[top] if A is None else A,
                             rel_q16(DEFAULTS["tolerance_rel"]) if Rq is None else Rq, pattern, top))
    for top in (255, 65535, 10000):
        rows.append((SCENE_T, SCENE_H, SCENE_W, 2, 2, 2, 2, SCENE_TOLERANCE[top], rel_q16(0.02), "scene", top))
    return rows


@functools.lru_cache(maxsize=None)
def sequence(T, h, w, pattern, top, seed=1):
    """(T, h, w) codes of a pattern, u8 for top 255 and u16 otherwise, read-only"""
    shape = (T, h, w)
    g = np.random.default_rng([seed, T, h, w, top, PATTERNS.index(pattern)])
    levels = np.array([top // 4, top // 2, 3 * (top // 4)] if pattern != "high" else [33000, 45000, 60000], dtype=np.int64)
    base = levels[g.integers(0, 3, size=(h, w))]                 # a static level per pixel ...
    noisy = np.clip(base[None] + g.integers(-2, 3, size=shape), 1, top)       # ... under fresh noise in every frame
    if pattern in ("random", "high"):       # 30 % holes, and one sample in twenty on another level: a spike
        c = np.where(g.random(shape) < 0.05, levels[g.integers(0, 3, size=shape)], noisy)
        c[g.random(shape) < 0.3] = 0
        if pattern == "high":
            assert top == 65535
            c.flat[0] = 65535
    elif pattern == "all":
        c = noisy
    elif pattern == "none":
        c = np.zeros(shape, dtype=np.int64)
    elif pattern == "scene":                # the scene, tiled and cropped in space and repeated in time
        s = scene(top)[0].astype(np.int64)
        c = np.tile(s, (-(-T // SCENE_T), -(-h // SCENE_H), -(-w // SCENE_W)))[:T, :h, :w]
    else:                                   # every pixel valid in exactly one frame
        assert pattern == "single"
        c = np.where(np.arange(T)[:, None, None] == g.integers(0, T, size=(h, w))[None], noisy, 0)
    out = c.astype(np.uint8 if top == 255 else np.uint16)
    assert np.array_equal(out, c) and out.shape == shape
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def want(case):
    """(codes, stats) of a case, computed once, read-only"""
    T, h, w, Bk, Ah, M, F, A, Rq, pattern, top = case
    out, stats = temporal(sequence(T, h, w, pattern, top), Bk, Ah, A, Rq, M, F)
    out.setflags(write=False)
    stats.setflags(write=False)
    return out, stats


# codon_temporal_depth's refusals, in the order the entry checks them: (what differs from a good call of u16 codes on three 5 x 7
# frames, a piece of the message)
REFUSALS = [({"src": None}, "null pointer"), ({"out": None}, "null pointer"),
            ({"T": 0}, "frames 0 "), ({"T": 4097}, "frames 4097 "),
            ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"), ({"h": 4097}, "a 4097x7 plane"), ({"w": 4097}, "a 5x4097 plane"),
            ({"T": 128, "h": 4096, "w": 4096}, "a sequence of 2147483648 codes"), ({"T": 4096, "h": 4096, "w": 4096}, "a sequence of 68719476736 codes"),
            ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "),
            ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "), ({"fmt": 0, "top": 1000}, "top 1000 "),
            ({"back": -1}, "window back -1 ahead 2"), ({"ahead": -1}, "window back 2 ahead -1"), ({"back": 8, "ahead": 7}, "window back 8 ahead 7"),
            ({"back": 15, "ahead": 0}, "window back 15 ahead 0"),
            ({"tol_abs": -1}, "tolerance -1 "), ({"top": 10000, "tol_abs": 10001}, "tolerance 10001 "),
            ({"tol_rel": -1}, "tolerance_rel -1 "), ({"tol_rel": 65536}, "tolerance_rel 65536 "),
            ({"count": 0}, "min_count 0 "), ({"count": 16}, "min_count 16 "),
            ({"fill": -1}, "min_fill -1 "), ({"fill": 16}, "min_fill 16 "),
            ({"out": "src"}, "same buffer")]
