"""numpy restatement of the hole-aware bicubic resampling (codon_amd/csrc/resample_masked.hip) -- TEST
INFRASTRUCTURE.  There is no reference for any of it; the kernels must match this BIT FOR BIT.  0.0 (code 0) is a hole.

The numerator IS the unmasked arithmetic on the plane (holes entering as 0.0) and the denominator the same arithmetic on the
validity plane, so both come from the existing restatements used unchanged: oracle/upsample_oracle.py for the upsample,
tests/train_data_ref.py for the downsample.  What is stated here is the count of invalid taps, the three-way rule, the snap onto
the code grid and the fused codes -> input composition."""
import numpy as np

from oracle import upsample_oracle as U
from tests import train_data16_ref as R16
from tests import train_data_ref as R

F = np.float32


def rule(N, D, invalid):
    """(value, valid, branch): branch 0 -- no invalid tap: N; 1 -- D >= 0.5: N / D (fp32 divide, correctly rounded); 2 -- hole."""
    N, D = np.asarray(N, dtype=F), np.asarray(D, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = N / D
    assert q.dtype == F
    branch = np.where(invalid == 0, 0, np.where(D >= F(0.5), 1, 2))
    out = np.where(branch == 0, N, np.where(branch == 1, q, F(0))).astype(F)
    return out, (branch != 2), branch


def _tap_counts_up(n, s):
    """(n*s, n) int64: how many of output index g's four clamped taps land on source index i (a clamped tap is a real tap)."""
    taps, _ = U.index_table(n, s)
    T = np.zeros((n * s, n), dtype=np.int64)
    for k in range(4):
        np.add.at(T, (np.arange(n * s), taps[:, k]), 1)
    return T


def upsample_masked(lr, s, with_branch=False):
    """lr (B,1,h,w) fp32, 0.0 a hole -> (out (B,1,h*s,w*s) fp32, valid bool)."""
    lr = np.asarray(lr, dtype=F)
    hole = lr[:, 0] == 0
    N = U.bicubic_upsample(lr, s)
    D = U.bicubic_upsample((~hole).astype(F)[:, None], s)
    Ty, Tx = _tap_counts_up(lr.shape[2], s), _tap_counts_up(lr.shape[3], s)
    invalid = np.einsum("gi,bij,xj->bgx", Ty, hole.astype(np.int64), Tx)[:, None]
    out, valid, branch = rule(N, D, invalid)
    return (out, valid, branch) if with_branch else (out, valid)


def _tap_counts_down(P, s):
    """(P/s, P) int64: 1 where input index i is one of output o's 4s taps INSIDE the image (out-of-image taps weigh 0)."""
    p = P // s
    A = np.zeros((p, P), dtype=np.int64)
    for o in range(p):
        for k in range(4 * s):
            i = o * s - 3 * s // 2 + k
            if 0 <= i < P:
                A[o, i] = 1
    return A


def snap(v, levels, lut):
    """A valid value as a sensor's file holds it: never code 0."""
    c = np.rint(np.clip(np.asarray(v, dtype=F), F(0), F(1)) * F(levels)).astype(np.int64)
    return np.asarray(lut, dtype=F)[np.clip(c, 1, levels)]


def downsample_masked(hr, s, levels, lut, with_branch=False):
    """hr (B,1,P,P) fp32, 0.0 a hole -> lr (B,1,P/s,P/s) on the code grid, holes +0.0."""
    hr = np.asarray(hr, dtype=F)
    hole = hr[:, 0] == 0
    N = R.downsample(hr, s)
    D = R.downsample((~hole).astype(F)[:, None], s)
    A = _tap_counts_down(hr.shape[2], s)
    invalid = np.einsum("oi,bij,xj->box", A, hole.astype(np.int64), A)[:, None]
    v, valid, branch = rule(N, D, invalid)
    out = np.where(valid, snap(v, levels, lut), F(0)).astype(F)
    return (out, branch) if with_branch else out


def tables(depth_bits, depth_max=65535):
    """(levels, lut) of a data set: 255 and the u8 table, or depth_max and lut16."""
    return (255, R.lut()) if depth_bits == 8 else (depth_max, R16.lut16(depth_max))


def quantize(x, levels, lut):
    v = np.clip(np.asarray(x, dtype=F), F(0), F(1)) * F(levels)
    assert v.dtype == F
    return np.asarray(lut, dtype=F)[np.rint(v).astype(np.int64)]


def cast_bits(x, dtype):
    """fp32 -> "f32": fp32; "f16": np.float16 (round to nearest even); "bf16": the uint16 bit patterns, nearest even."""
    x = np.asarray(x, dtype=F)
    if dtype == "f32":
        return x
    if dtype == "f16":
        return x.astype(np.float16)
    u = np.ascontiguousarray(x).view(np.uint32)
    return ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)


def codes_to_input(codes, s, levels, lut, dtype="f32"):
    """codes (B,h,w) integer -> the network's depth input (B,1,h*s,w*s) as cast_bits gives it."""
    v = np.asarray(lut, dtype=F)[np.asarray(codes).astype(np.int64)][:, None]
    up, _ = upsample_masked(v, s)
    return cast_bits(quantize(up, levels, lut), dtype)


def degrade(src, s, levels, lut):
    """(x, lr) of train.synthesize(degrade_holes=True) from the source crops (B,1,P,P)."""
    lr = downsample_masked(src, s, levels, lut)
    up, _ = upsample_masked(lr, s)
    return quantize(up, levels, lut), lr


# ---- the hole patterns of the tests -------------------------------------------------------------------------------------------

KINDS = ("none", "pattern", "rowcol", "borders", "all", "one")


def holes(h, w, kind, seed=0):
    """(h,w) bool, True = hole.  "pattern": 6 % isolated holes plus one 4 x 5 blob (clipped to the plane), seeded."""
    g = np.random.default_rng(seed)
    m = np.zeros((h, w), dtype=bool)
    if kind == "pattern":
        m |= g.uniform(size=(h, w)) < 0.06
        y0, x0 = int(g.integers(0, max(h - 4, 1))), int(g.integers(0, max(w - 5, 1)))
        m[y0:y0 + 4, x0:x0 + 5] = True
    elif kind == "rowcol":
        m[h // 2, :] = True
        m[:, w // 3] = True
    elif kind == "borders":
        m[0, :] = m[-1, :] = True
        m[:, 0] = m[:, -1] = True
    elif kind == "all":
        m[:] = True
    elif kind == "one":
        m[:] = True
        m[h // 2, w // 2] = False
    elif kind != "none":
        raise ValueError(kind)
    return m


def plane(B, h, w, kind, seed=0, levels=None):
    """(B,1,h,w) fp32 in (0, 1] with that pattern of holes (another seed per image); levels: values on the code grid."""
    g = np.random.default_rng(1000 + seed)
    if levels is None:
        v = g.uniform(0.05, 1.0, size=(B, 1, h, w)).astype(F)
    else:
        lut = R.lut() if levels == 255 else R16.lut16(levels)
        v = lut[g.integers(1, levels + 1, size=(B, 1, h, w))]
    for b in range(B):
        v[b, 0][holes(h, w, kind, seed + b)] = 0
    return v
