"""numpy restatement of the surface-normal angle error (codon_amd/csrc/normal_errors.hip, codon_amd.metrics.normal_errors; DESIGN
12.20) and the inputs its tests share -- TEST INFRASTRUCTURE.  The kernel is held to these words and maps, no tolerance.  A
DEFINITION of this project.

Label and output are code planes, 0 a hole; the label is at least as large as the output and is read top-left.  Inside the H x W
window the output counts as 0 wherever the label is 0.  N_l, N_o: tests/cloud_ref.py's normals_q14 (imported, not restated) of the
label window and of the masked output under the first W and H rays.  A pixel is COMPARED when its label is non-zero and both have
a normal.  For a compared pixel D = N_l . N_o, X = |N_l x N_o|^2, A = isqrt(X), and with C[m] = rint(2^30 cos t_m), S[m] =
rint(2^30 sin t_m), t_m = (m - 1/2) / 8 degrees, m = 1 .. 1440: a = #{ m : A C[m] - D S[m] > 0 }.
Per image 1448 u32 words: 0 .. 1440 the histogram of a over the compared pixels, 1441 valid label pixels in the window, 1442 those
whose label has a normal, 1443 compared pixels, 1444 pixels with label != 0 and output == 0, 1445 .. 1447 zero.  Angle map: a where
compared, 65535 elsewhere."""
import functools
import math

import numpy as np

from tests import cloud_ref as Q
from tests.clean_ref import rel_q16
from tests.cloud_ref import normals_q14

ANGLES, BINS, WORDS = 1440, 1441, 1448
VALID, LABEL_NORMALS, COMPARED, OUT_HOLES = 1441, 1442, 1443, 1444
NONE = 65535
S_MIN = 1171270                              # rint(2^30 sin(1/16 degree))


@functools.lru_cache(maxsize=None)
def angle_tables():
    """(C, S) int64 (1440 each), entry m - 1 for threshold m"""
    t = np.radians((np.arange(1, ANGLES + 1, dtype=np.float64) - 0.5) / 8.0)
    c, s = np.rint(float(1 << 30) * np.cos(t)).astype(np.int64), np.rint(float(1 << 30) * np.sin(t)).astype(np.int64)
    c.setflags(write=False), s.setflags(write=False)
    return c, s


def isqrt(v):
    return np.array([math.isqrt(int(x)) for x in np.asarray(v).ravel()], dtype=np.int64).reshape(np.shape(v))


def dot_and_root(p, q):
    """(D, A) int64 of (n, 3) Q14 normals"""
    p, q = np.asarray(p, dtype=np.int64), np.asarray(q, dtype=np.int64)
    D = (p * q).sum(axis=-1)
    x = np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                  p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], axis=-1)
    return D, isqrt((x * x).sum(axis=-1))


def index_count(p, q):
    """THE DEFINITION: a = #{ m : A C[m] - D S[m] > 0 } of (n, 3) normals -> (n) int64"""
    C, S = angle_tables()
    D, A = dot_and_root(p, q)
    out = np.zeros(D.shape, dtype=np.int64)
    for lo in range(0, D.size, 4096):                                   # 4096 x 1440 int64 at a time
        d, a = D.ravel()[lo:lo + 4096, None], A.ravel()[lo:lo + 4096, None]
        out.ravel()[lo:lo + 4096] = (a * C[None] - d * S[None] > 0).sum(axis=1)
    return out


def index_bisect(p, q):
    """What the kernel does: the largest m whose predicate holds by a greedy descent in 11 steps, 0 if none"""
    C, S = angle_tables()
    D, A = dot_and_root(p, q)
    a = np.zeros(D.shape, dtype=np.int64)
    for step in (1024, 512, 256, 128, 64, 32, 16, 8, 4, 2, 1):
        m = a + step
        at = np.minimum(m, ANGLES) - 1
        a = np.where((m <= ANGLES) & (A * C[at] - D * S[at] > 0), m, a)
    return a


def normal_errors_plane(label, out, rx, ry, radius, tolerance, Rq):
    """(words (1448) uint32, angle map (H, W) uint16) of one label (Hl, Wl) and one output (H, W)"""
    label, out = np.asarray(label), np.asarray(out)
    label = label.view(np.uint16) if label.dtype == np.int16 else label
    out = out.view(np.uint16) if out.dtype == np.int16 else out
    H, W = out.shape
    assert label.shape[0] >= H and label.shape[1] >= W and len(rx) >= W and len(ry) >= H
    l = label[:H, :W].astype(np.int64)
    o = np.where(l != 0, out.astype(np.int64), 0)
    Nl, hl = normals_q14(l, rx[:W], ry[:H], radius, tolerance, Rq)
    No, ho = normals_q14(o, rx[:W], ry[:H], radius, tolerance, Rq)
    cmp = (l != 0) & hl & ho
    a = index_count(Nl[cmp], No[cmp])
    words = np.zeros(WORDS, dtype=np.uint32)
    words[:BINS] = np.bincount(a, minlength=BINS)
    words[VALID], words[LABEL_NORMALS], words[COMPARED] = (l != 0).sum(), ((l != 0) & hl).sum(), cmp.sum()
    words[OUT_HOLES] = ((l != 0) & (out == 0)).sum()
    amap = np.full((H, W), NONE, dtype=np.uint16)
    amap[cmp] = a
    return words, amap


def normal_errors(label, out, rx, ry, radius, tolerance, Rq):
    """normal_errors_plane over a batch -> ((B, 1448) uint32, (B, H, W) uint16)"""
    r = [normal_errors_plane(l, o, rx, ry, radius, tolerance, Rq) for l, o in zip(np.asarray(label), np.asarray(out))]
    return np.stack([x[0] for x in r]), np.stack([x[1] for x in r])


def report(words, thresholds=(11.25, 22.5, 30.0)):
    """metrics.normal_report restated: degrees"""
    w = [int(v) for v in words]
    hist, n, valid = w[:BINS], w[COMPARED], w[VALID]
    r = {"normal_n": n, "normal_coverage": n / valid if valid else math.nan}
    nan = math.nan
    cum = np.cumsum(hist)
    r["normal_mean"] = sum(a * v for a, v in enumerate(hist)) / (8 * n) if n else nan
    r["normal_rmse"] = math.sqrt(sum(a * a * v for a, v in enumerate(hist)) / n) / 8 if n else nan
    r["normal_median"] = int(np.argmax(cum >= (n + 1) // 2)) / 8 if n else nan
    for t in thresholds:
        r[f"normal<{t:g}"] = int(cum[int(8 * t)]) / n if n else nan
    return r


# ---- the shared cases of the GPU test and of the host-side check ----------------------------------------------------------------------

# (B, h, w): one pixel; a single row; odd sizes, where nothing is compared at radius 8; exactly one tile; a second tile of one pixel
# each way, so the halo crosses tile borders; a batch, for the per-image rows; many tiles, the label a window of a larger plane
SHAPES = ((1, 1, 1), (1, 1, 37), (1, 5, 7), (1, 32, 32), (1, 33, 33), (3, 9, 33), (1, 93, 116))
WINDOWED = SHAPES[6]
PAD = (5, 7)                                 # the rows and columns of the larger plane beyond the window
RADII = (1, 2, 8)
NOISES = ("0", "1", "wide")                  # the output is the label plus integer noise of amplitude 0, 1, top // 100, clipped
PATTERNS = ("random", "u8", "high", "surfaces", "checker", "none")


def amplitude(noise, top):
    return {"0": 0, "1": 1, "wide": top // 100}[noise]


def cases(shape):
    """[(pattern, radius, noise, holes)] of a shape; holes: the output is 0 at a tenth of the valid label pixels (word 1444)"""
    out = []
    for pattern in PATTERNS:
        noises = NOISES if pattern in ("random", "u8", "high", "surfaces") else ("0", "wide") if pattern == "checker" else ("0",)
        out += [(pattern, radius, noise, False) for radius in RADII for noise in noises]
    return out + [("random", radius, "1", True) for radius in RADII]


def tolerance_of(top):
    return max(2, top // 500)


RQ = rel_q16(Q.DEFAULTS["tolerance_rel"])


def label_shape(shape):
    B, h, w = shape
    return (B, h + PAD[0], w + PAD[1]) if tuple(shape) == WINDOWED else (B, h, w)


@functools.lru_cache(maxsize=None)
def tables(shape):
    """The rays of the LABEL's camera: the window uses their first w and h entries"""
    _, hl, wl = label_shape(shape)
    rx, ry = Q.ray_tables(wl, hl, *Q.camera_of(shape))
    rx.setflags(write=False), ry.setflags(write=False)
    return rx, ry


@functools.lru_cache(maxsize=None)
def planes(shape, pattern, noise, holes=False):
    """(label (B, hl, wl), output (B, h, w)) of a case, read-only: the label is cloud_ref.plane in the top-left window of a plane
    of non-zero codes; the output is the label plus noise, clipped into 1 .. top -- and ANY code where the label is a hole, which
    the mask must keep from being read as a surface"""
    B, h, w = shape
    top = Q.top_of(pattern)
    window = Q.plane(shape, pattern).astype(np.int64)
    g = np.random.default_rng([11, B, h, w, PATTERNS.index(pattern), NOISES.index(noise), int(holes)])
    label = g.integers(1, top + 1, size=label_shape(shape))
    label[:, :h, :w] = window
    amp = amplitude(noise, top)
    out = np.clip(window + g.integers(-amp, amp + 1, size=shape), 1, top)
    out = np.where(window != 0, out, g.integers(1, top + 1, size=shape))
    if holes:
        out = np.where(g.uniform(size=shape) < 0.1, 0, out)
    dt = np.uint8 if top == 255 else np.uint16
    label, out = label.astype(dt), out.astype(dt)
    label.setflags(write=False), out.setflags(write=False)
    return label, out


@functools.lru_cache(maxsize=None)
def want(shape, pattern, radius, noise, holes=False):
    """((B, 1448) uint32, (B, h, w) uint16) of a case, computed once, with the asserts that keep the cases from going idle"""
    label, out = planes(shape, pattern, noise, holes)
    rx, ry = tables(shape)
    words, maps = normal_errors(label, out, rx, ry, radius, tolerance_of(Q.top_of(pattern)), RQ)
    bins = [np.flatnonzero(w[:BINS]) for w in words]
    valid = (Q.plane(shape, pattern) != 0).reshape(shape[0], -1).sum(axis=1)
    for b in range(shape[0]):
        assert words[b, VALID] == valid[b] and words[b, :BINS].sum() == words[b, COMPARED] <= words[b, LABEL_NORMALS] <= valid[b]
        if noise == "0" and not holes:
            assert bins[b].size == 0 or bins[b].tolist() == [0], (shape, pattern, radius, "a plane against itself leaves bin 0")
            assert words[b, COMPARED] == words[b, LABEL_NORMALS]
        if noise == "wide" and radius <= 2 and pattern in ("random", "u8", "high") and valid[b] >= 500:
            assert bins[b].size >= 64, (shape, pattern, radius, bins[b].size, "the wide cases spread over 64 bins or more")
    if tuple(shape) == WINDOWED and pattern == "random" and noise == "wide" and radius <= 2:
        assert bins[0].max() > 720, "the 93 x 116 random case reaches past 90 degrees"
    if pattern == "checker" and radius == 1:                           # the pixels one step away are holes
        assert (words[:, COMPARED] == 0).all() and (words[:, VALID] > 0).all()
    if pattern == "checker" and radius == 2 and noise == "0" and min(shape[1:]) >= 3:
        assert (words[:, COMPARED] == valid).all()                      # those two steps away are valid and linked
    if holes:
        assert (words[:, OUT_HOLES] > 0).all() or shape[1] * shape[2] < 40
    words.setflags(write=False), maps.setflags(write=False)
    return words, maps


# codon_normal_errors' refusals: (what differs from a good call of u16 codes on a 5 x 7 window of a 6 x 9 label, a piece of the message)
REFUSALS = [({"label": None}, "null pointer"), ({"out": None}, "null pointer"), ({"rx": None}, "null pointer"),
            ({"ry": None}, "null pointer"), ({"span": None}, "null pointer"), ({"ctab": None}, "null pointer"),
            ({"stab": None}, "null pointer"), ({"words": None}, "null pointer"),
            ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "), ({"B": 0}, "batch 0 "), ({"B": 65536}, "batch 65536 "),
            ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"), ({"h": 4097, "hl": 4097}, "a 4097x7 plane"),
            ({"w": 4097, "wl": 4097}, "a 5x4097 plane"),
            ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "), ({"fmt": 0, "top": 1000}, "top 1000 "),
            ({"hl": 4}, "a 4x9 label is smaller than the 5x7 output"), ({"wl": 6}, "a 6x6 label is smaller than the 5x7 output"),
            ({"row": 8}, "label strides 8 (row)"), ({"B": 2, "image": 40}, "label strides 9 (row), 40 (image)"),
            ({"image": -1}, "label strides 9 (row), -1 (image)"),
            ({"radius": 0}, "radius 0 "), ({"radius": 9}, "radius 9 "),
            ({"tol_abs": -1}, "tolerance -1 "), ({"top": 10000, "tol_abs": 10001}, "tolerance 10001 "),
            ({"tol_rel": -1}, "tolerance_rel -1 "), ({"tol_rel": 65536}, "tolerance_rel 65536 "),
            ({"span": (0, 1 << 22, 0, 0)}, "ray 1 of the span is 4194304"), ({"span": (0, 0, -(1 << 22), 0)}, "ray 2 of the span is -4194304")]


# ---- pairs of normals that no scene reaches ------------------------------------------------------------------------------------------

def _units(g, n):
    v = g.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


@functools.lru_cache(maxsize=None)
def pairs(n_random=20000, per_threshold=4, seed=5):
    """(n, 6) int32, two Q14 normals a row: random directions (half of them with D < 0), pairs placed on every threshold t_m as
    closely as Q14 allows, identical pairs and opposite pairs; (the rows of each kind) beside them"""
    g = np.random.default_rng(seed)
    q14 = lambda v: np.rint(16384.0 * v).astype(np.int64)                                           # noqa: E731
    rnd = np.concatenate([q14(_units(g, n_random)), q14(_units(g, n_random))], axis=1)
    t = np.radians((np.repeat(np.arange(1, ANGLES + 1), per_threshold) - 0.5) / 8.0)[:, None]
    p = _units(g, len(t))
    side = np.cross(p, _units(g, len(t)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    on = np.concatenate([q14(p), q14(np.cos(t) * p + np.sin(t) * side)], axis=1)
    u = q14(_units(g, 64))
    rows = np.concatenate([rnd, on, np.concatenate([u, u], axis=1), np.concatenate([u, -u], axis=1)]).astype(np.int32)
    kinds = {"random": slice(0, n_random), "threshold": slice(n_random, n_random + len(on)),
             "same": slice(n_random + len(on), n_random + len(on) + 64), "opposite": slice(n_random + len(on) + 64, len(rows))}
    rows.setflags(write=False)
    return rows, kinds
