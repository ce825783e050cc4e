"""numpy restatement of the depth evaluation suite (codon_amd/csrc/eval.hip, codon_amd.metrics.depth_errors) --
TEST INFRASTRUCTURE.  The reference prints one masked RMSE and one SSIM per image and nothing else, so this is the definition;
the kernel must match it BIT FOR BIT (everything is an integer).  tests/test_eval_cpu.py pins it on hand-worked cases.

One image: a label plane L (uint8 or uint16, at least as large as the output, read top-left) and an output plane O (H, W) of the
same type.  valid v = (L != 0), e = |L - O|.  Sixteen uint64 words:
  0 n = #v | 1 sum_v e | 2 sum_v e^2 | 3 max_v e (0 when n = 0) | 4-7 #{v, e > t_k} (unused: 0)
  8-10 #{v, 4 max(L,O) < 5 min(L,O)}, 16 max < 25 min, 64 max < 125 min (O = 0 never an inlier)
  11 n_E | 12 sum_E e | 13 sum_E e^2 | 14-15 0
Edge region E: a pixel is a discontinuity when it is valid and some 4-neighbour INSIDE the H x W window is valid and differs by
more than T; E = the valid pixels within Chebyshev distance r of a discontinuity.  Label pixels beyond the window do not exist
for this purpose.  Edge evaluation off (edge_threshold None): words 11-13 are 0.
Maps: error map (the codes' type) e where valid, 0 elsewhere; region map (uint8) 0 hole, 1 valid outside E, 2 valid in E."""
import math

import numpy as np

WORDS = 16
MAX_THRESHOLDS = 4
MAX_RADIUS = 8


def discontinuities(L, T):
    """bool (H, W): valid pixels with a valid 4-neighbour inside the plane that differs by more than T."""
    L = np.asarray(L).astype(np.int64)
    v = L != 0
    d = np.zeros(L.shape, dtype=bool)
    H, W = L.shape
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
        xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
        # p at [yd, xd], its neighbour q = p + (dy, dx) at [ys, xs]
        d[yd, xd] |= v[yd, xd] & v[ys, xs] & (np.abs(L[yd, xd] - L[ys, xs]) > T)
    return d


def dilate(d, r):
    """bool: pixels within Chebyshev distance r of a True pixel of d (the plane's border cuts the window)."""
    H, W = d.shape
    out = np.zeros_like(d)
    for y, x in zip(*np.nonzero(d)):
        out[max(y - r, 0):min(y + r + 1, H), max(x - r, 0):min(x + r + 1, W)] = True
    return out


def depth_errors(label, out, thresholds=(), edge_threshold=None, edge_radius=1):
    """-> (words uint64[16], error map of out's dtype (H, W), region map uint8 (H, W)) of ONE image."""
    label, out = np.asarray(label), np.asarray(out)
    assert label.dtype == out.dtype and out.dtype in (np.uint8, np.uint16) and out.ndim == 2 and label.ndim == 2
    H, W = out.shape
    assert label.shape[0] >= H and label.shape[1] >= W and len(thresholds) <= MAX_THRESHOLDS
    L = label[:H, :W].astype(np.int64)
    O = out.astype(np.int64)
    v = L != 0
    e = np.where(v, np.abs(L - O), 0)
    w = [0] * WORDS
    w[0] = int(v.sum())
    w[1] = int(e.sum())
    w[2] = int((e * e).sum())
    w[3] = int(e.max()) if w[0] else 0
    for k, t in enumerate(thresholds):
        assert int(t) == t and t >= 0
        w[4 + k] = int((v & (e > t)).sum())
    mx, mn = np.maximum(L, O), np.minimum(L, O)
    for k, (p, q) in enumerate(((4, 5), (16, 25), (64, 125))):
        w[8 + k] = int((v & (p * mx < q * mn)).sum())
    region = v.astype(np.uint8)
    if edge_threshold is not None:
        assert 0 <= edge_radius <= MAX_RADIUS and edge_threshold >= 0
        E = v & dilate(discontinuities(L, edge_threshold), edge_radius)
        w[11] = int(E.sum())
        w[12] = int(e[E].sum())
        w[13] = int((e[E] * e[E]).sum())
        region[E] = 2
    return np.array(w, dtype=np.uint64), e.astype(out.dtype), region


def depth_errors_batch(label, out, **kw):
    """(B, 16) words, (B, H, W) error maps, (B, H, W) region maps of (B, ., .) planes."""
    r = [depth_errors(l, o, **kw) for l, o in zip(label, out)]
    return tuple(np.stack([x[k] for x in r]) for k in range(3))


def _div(a, b):
    return a / b if b else math.nan


def depth_report(words, unit=1.0, thresholds=()):
    """The host arithmetic of codon_amd.metrics.depth_report, restated: Python ints and floats only."""
    w = [int(x) for x in words]
    n, nE = w[0], w[11]
    r = {"n": n, "mad": w[1] / n * unit, "rmse": math.sqrt(w[2] / n) * unit, "max": w[3] * unit}
    for k, t in enumerate(thresholds):
        r[f"bad>{t}"] = w[4 + k] / n
    r.update(delta1=w[8] / n, delta2=w[9] / n, delta3=w[10] / n, edge_fraction=nE / n)
    r["edge_mad"] = _div(w[12], nE) * unit
    r["edge_rmse"] = math.sqrt(_div(w[13], nE)) * unit
    r["flat_mad"] = _div(w[1] - w[12], n - nE) * unit
    r["flat_rmse"] = math.sqrt(_div(w[2] - w[13], n - nE)) * unit
    return r


# ---- test inputs (shared by tests/test_eval_cpu.py, tests/test_gpu_eval.py and tools/host_check.py) ---------------------

SHAPES = ((1, 5, 7), (1, 32, 32), (1, 33, 70), (3, 37, 53))       # B x H x W: below one halo, exactly one tile, ragged, a batch
RADII = (0, 1, 3, 8)
PARAMS = {8: {"thresholds": (0, 1, 3, 5), "edge_threshold": 20}, 16: {"thresholds": (0, 200, 600, 1000), "edge_threshold": 4000}}
DTYPE = {8: np.uint8, 16: np.uint16}
FACTORS = (0.45, 0.6, 0.75, 1.3)         # outliers: fails delta3 | fails delta2, passes delta3 | fails delta1, passes delta2 (twice)
PAD = (3, 5)                             # the label is this much larger than the output


def case(shape, bits, seed=0):
    """(label (B, H + 3, W + 5), out (B, H, W)) of DTYPE[bits], deterministic.  Label: piecewise constant on blocks of 16 x 23
    pixels (the grid shifted so that a 5 x 7 image still straddles four blocks), steps of 60 codes (8-bit; 200 times that for
    16-bit) plus 0-2 codes of jitter, about 10 % holes.  Output: the clean steps +- 6 codes, about 15 % outliers at FACTORS of
    the label, about 2 % at code 0."""
    B, H, W = shape
    s = 1 if bits == 8 else 200
    top = 255 if bits == 8 else 65535
    g = np.random.default_rng([seed, bits, B, H, W])
    Hl, Wl = H + PAD[0], W + PAD[1]
    by, bx = (np.arange(Hl) + 13) // 16, (np.arange(Wl) + 19) // 23
    levels = g.integers(0, 4, size=(B, by.max() + 1, bx.max() + 1))
    clean = (40 + 60 * levels[:, by[:, None], bx[None, :]]) * s
    label = clean + g.integers(0, 2 * s, size=clean.shape, endpoint=True)
    label[g.uniform(size=clean.shape) < 0.10] = 0
    out = clean[:, :H, :W] + g.integers(-6 * s, 6 * s, size=(B, H, W), endpoint=True)
    u = g.uniform(size=(B, H, W))
    f = np.asarray(FACTORS)[g.integers(0, len(FACTORS), size=(B, H, W))]
    out = np.where(u < 0.15, np.rint(label[:, :H, :W] * f).astype(np.int64), out)
    out[(u >= 0.15) & (u < 0.17)] = 0
    return label.astype(DTYPE[bits]), np.clip(out, 0, top).astype(DTYPE[bits])
