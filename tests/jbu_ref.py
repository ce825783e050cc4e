"""numpy restatement of the joint bilateral upsampler (codon_amd/csrc/jbu.hip, codon_amd.upsample.joint_bilateral_upsample;
DESIGN 12.14) and the inputs its tests share -- TEST INFRASTRUCTURE.  Integers only: the kernel is held to these bits, no
tolerance.  A DEFINITION of this project after Kopf et al. 2007, on the bicubic's own 4 x 4 footprint.

Codes c (h x w, 0 a hole; u8 with top 255 or u16), guidance g (u8, the top-left h s x w s of it), scale s in 4, 8, 16, range table T
(256 entries in 1 .. 256), spatial table S (s x 4 entries in 1 .. 256).  G_0 = guided_fill_ref.guide_base(g, h, w, s).  For the
high-resolution pixel (Y, X), with floor division: y0 = (2 Y + 1 - s) // (2 s), rows y0 - 1 .. y0 + 2 (tap ky = 0 .. 3), columns
likewise.  S[ph][k] = max(1, rint(256 exp(-d^2 / (2 sigma_s^2)))) with d = |t(ph) - 2 s (k - 1)| / (2 s), the tap's distance in
low-resolution pixels, t(ph) = (2 ph + 1 - s) mod 2 s.  Tap q = (yy, xx) weighs
    w_q = max(1, (S[Y mod s][ky] S[X mod s][kx] + 128) >> 8) T[|g(Y, X) - G_0(q)|]      (at most 2^16),
0 where q lies outside the plane or c(q) = 0, and out(Y, X) = (2 sum w_q c(q) + sum w_q) // (2 sum w_q), 0 (a hole) exactly where
no tap of the footprint is valid."""
import functools

import numpy as np

from tests import fill_ref as F
from tests import guided_fill_ref as R

SCALES = R.SCALES
SIGMA_S = 1.0
SIGMAS_S = (0.5, 1.0)
# sum w_q <= 16 * 2^16 = 2^20, so the numerator 2 sum w c + sum w is at most this: 64 bits for u16 codes, and with u8 codes
# 2 * 2^20 * 255 + 2^20 < 2^30
WEIGHT_SUM_MAX = 16 << 16
NUMERATOR_MAX = 2 * WEIGHT_SUM_MAX * 65535 + WEIGHT_SUM_MAX
NUMERATOR_MAX_U8 = 2 * WEIGHT_SUM_MAX * 255 + WEIGHT_SUM_MAX
assert 1 << 31 < NUMERATOR_MAX < 1 << 38 and NUMERATOR_MAX_U8 < 1 << 30

# codon_jbu_upsample's refusals: (what differs from a good call of u16 codes on a 5 x 7 plane at x4, a piece of the message) --
# codon_fill_holes_guided's, word for word, and the spatial table
REFUSALS = R.REFUSALS[:5] + [({"stab": None}, "null pointer")] + R.REFUSALS[5:]


@functools.lru_cache(maxsize=None)
def _spatial_table(s, sigma_s):
    t = np.zeros((s, 4), dtype=np.uint16)
    for ph in range(s):
        num = (2 * ph + 1 - s) % (2 * s)
        for k in range(4):
            d = abs(num - 2 * s * (k - 1)) / (2.0 * s)
            t[ph, k] = max(1.0, np.rint(256.0 * np.exp(-d * d / (2.0 * float(sigma_s) ** 2))))
    t.setflags(write=False)
    return t


def spatial_table(s, sigma_s=SIGMA_S):
    """S as (s, 4) uint16, float64 on the host"""
    return _spatial_table(int(s), float(sigma_s))


def taps(n, s):
    """(n s, 4) int64: the four low-resolution indices y0 - 1 .. y0 + 2 of every high-resolution index (not clamped)"""
    Y = np.arange(n * s, dtype=np.int64)
    y0 = (2 * Y + 1 - s) // (2 * s)
    return y0[:, None] + np.arange(-1, 3)[None, :]


def upsample_plane(c, g, s, T, S, with_sums=False):
    """out (h s, w s) of one plane of codes and its guidance, in the plane's dtype.  with_sums: (out, the largest numerator)"""
    c = np.asarray(c)
    h, w = c.shape
    T, S = np.asarray(T).astype(np.int64), np.asarray(S).astype(np.int64)
    assert T.shape == (256,) and T.min() >= 1 and T.max() <= 256 and s in SCALES
    assert S.shape == (s, 4) and S.min() >= 1 and S.max() <= 256
    G0 = R.guide_base(g, h, w, s).astype(np.int32)
    gh = np.asarray(g)[:h * s, :w * s].astype(np.int32)
    ci = c.astype(np.int32)
    T32, S32 = T.astype(np.int32), S.astype(np.int32)
    ty, tx = taps(h, s), taps(w, s)
    phy, phx = np.arange(h * s) % s, np.arange(w * s) % s
    num = np.zeros((h * s, w * s), dtype=np.int64)
    den = np.zeros((h * s, w * s), dtype=np.int64)
    for ky in range(4):
        iy = ty[:, ky]
        oky = (iy >= 0) & (iy < h)
        iyc = np.clip(iy, 0, h - 1)
        for kx in range(4):
            ix = tx[:, kx]
            okx = (ix >= 0) & (ix < w)
            ixc = np.clip(ix, 0, w - 1)
            cq = np.where(oky[:, None] & okx[None, :], ci[np.ix_(iyc, ixc)], 0)       # outside the plane: as a hole
            ws = np.maximum(1, (S32[phy, ky][:, None] * S32[phx, kx][None, :] + 128) >> 8)
            wq = ws * T32[np.abs(gh - G0[np.ix_(iyc, ixc)])]                          # int32: at most 2^16
            assert wq.max() <= 1 << 16
            wq[cq == 0] = 0
            num += wq.astype(np.int64) * cq
            den += wq
    top_num = int((2 * num + den).max())
    assert den.max() <= WEIGHT_SUM_MAX and top_num <= (NUMERATOR_MAX_U8 if c.dtype == np.uint8 else NUMERATOR_MAX)
    res = np.where(den > 0, (2 * num + den) // np.maximum(2 * den, 1), 0)
    out = res.astype(c.dtype)
    assert np.array_equal(out, res)
    return (out, top_num) if with_sums else out


def upsample(c, g, s, T, S):
    """upsample_plane over a (B, h, w) batch with (B, H, W) guidance"""
    return np.stack([upsample_plane(p, q, s, T, S) for p, q in zip(np.asarray(c), np.asarray(g))])


def footprint_valid(c, s):
    """(h s, w s) bool: the pixel's footprint holds a valid code; and the min and max of its valid taps (0 where none)"""
    c = np.asarray(c).astype(np.int64)
    h, w = c.shape
    ty, tx = taps(h, s), taps(w, s)
    big = np.iinfo(np.int64).max
    lo = np.full((h * s, w * s), big, dtype=np.int64)
    hi = np.zeros((h * s, w * s), dtype=np.int64)
    for ky in range(4):
        oky = (ty[:, ky] >= 0) & (ty[:, ky] < h)
        for kx in range(4):
            okx = (tx[:, kx] >= 0) & (tx[:, kx] < w)
            cq = c[np.ix_(np.clip(ty[:, ky], 0, h - 1), np.clip(tx[:, kx], 0, w - 1))]
            ok = oky[:, None] & okx[None, :] & (cq != 0)
            lo = np.where(ok, np.minimum(lo, cq), lo)
            hi = np.where(ok, np.maximum(hi, cq), hi)
    any_ = hi > 0
    return any_, np.where(any_, lo, 0), hi


# ---- the high-resolution occlusion scene ----------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def hr_scene(h, w, s, top, seed=3):
    """(codes, holed codes, guide, hr truth, near_hr) of guided_fill_ref.scene: codes its low-resolution truth (no holes), holed
    its codes with the hole band, truth the scene's edge rendered at high resolution, near top // 4 and far 3 top // 4"""
    holed, guide, codes = R.scene(h, w, s, top, seed)
    Y, X = np.mgrid[0:h * s, 0:w * s]
    near = X / s < R.edge_of(Y / s, w)
    truth = np.where(near, top // 4, 3 * top // 4).astype(codes.dtype)
    truth.setflags(write=False)
    near.setflags(write=False)
    return codes, holed, guide, truth, near


def edge_region(near, s):
    """The high-resolution pixels within s / 2 (Chebyshev) of a near / far boundary: a pixel whose 4-neighbour is on the other
    side is on the boundary"""
    near = np.asarray(near)
    b = np.zeros(near.shape, dtype=bool)
    dv, dh = near[1:] != near[:-1], near[:, 1:] != near[:, :-1]
    b[1:] |= dv
    b[:-1] |= dv
    b[:, 1:] |= dh
    b[:, :-1] |= dh
    r = s // 2
    H, W = b.shape
    p = np.zeros((H + 2 * r, W + 2 * r), dtype=bool)
    p[r:r + H, r:r + W] = b
    out = np.zeros_like(b)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def mad(a, b, where):
    return float(np.abs(np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64))[where].mean())


def bicubic_codes(codes, s, top):
    """(B, h s, w s) codes: the integer resample_masked_ref.codes_to_input looks up, rint(clamp(masked bicubic) top), which is
    upsample.bicubic_upsample_codes.  That restatement's own arithmetic (the oracle's bicubic for numerator and denominator, its
    rule) with the count of invalid taps as two matrix products, so that the large shapes take no seconds; the CPU test holds
    it to rint(codes_to_input(., "f32") levels) on the small ones."""
    from oracle import upsample_oracle as U
    from tests import resample_masked_ref as M
    codes = np.asarray(codes)
    levels, lut = M.tables(8 if codes.dtype == np.uint8 else 16, top)
    lr = np.asarray(lut, dtype=np.float32)[codes.astype(np.int64)][:, None]
    hole = lr[:, 0] == 0
    N = U.bicubic_upsample(lr, s)
    D = U.bicubic_upsample((~hole).astype(np.float32)[:, None], s)
    Ty, Tx = M._tap_counts_up(codes.shape[1], s), M._tap_counts_up(codes.shape[2], s)
    invalid = np.stack([Ty @ hb.astype(np.int64) @ Tx.T for hb in hole])[:, None]
    up, _, _ = M.rule(N, D, invalid)
    v = np.clip(up, np.float32(0), np.float32(1)) * np.float32(levels)
    assert v.dtype == np.float32
    return np.rint(v).astype(codes.dtype)[:, 0]


# ---- the shared cases: fill_ref's planes, guided_fill_ref's guides ---------------------------------------------------------------

FORMATS = (("u8", 255), ("u16", 65535), ("u16_10000", 10000))
CROSSED = tuple(F.SHAPES[:3])       # the small shapes run every pattern in every format; the others every pattern, the formats in turn


def cases(shape):
    """[(format name, top, pattern, kind of guidance, sigma_s, layout 0 .. 3)] of a fill_ref shape at guided_fill_ref.SHAPE_SCALE's
    scale: every shape sees every pattern, format, guide, sigma_s and layout of the guidance (the host check's four)"""
    out = []
    for pi, pattern in enumerate(F.PATTERNS):
        for fi, (name, top) in enumerate(FORMATS):
            if tuple(shape) not in CROSSED and fi != pi % 3:
                continue
            n = pi + fi
            out.append((name, top, pattern, R.GUIDES[n % 3], SIGMAS_S[n % 2], n % 4))
    return out


@functools.lru_cache(maxsize=None)
def want(shape, pattern, top, s, kind, table, sigma_s, seed=1):
    """upsample(fill_ref.case(...), guided_fill_ref.guide_case(...)), computed once.  sigma_s: a float, or "c<n>" the constant
    spatial table of n"""
    S = np.full((s, 4), int(sigma_s[1:]), dtype=np.uint16) if isinstance(sigma_s, str) else spatial_table(s, sigma_s)
    out = upsample(F.case(shape, pattern, top, seed), R.guide_case(tuple(shape), s, kind), s, R.table_of(table), S)
    out.setflags(write=False)
    return out
