"""numpy restatement of the sensor model of the training degradation (codon_amd/csrc/sensor.hip, sensor_pixel.h,
sensor_rng.h) -- TEST INFRASTRUCTURE.  There is no reference for any of it; the kernel must match this BIT FOR BIT.

Philox4x32-10 on uint64 arrays (every word kept below 2^32 by explicit masks), the Gaussian table from the standard library's
inverse normal CDF, and the per-pixel rule; the snap onto the code grid is tests/resample_masked_ref.snap, unchanged."""
import functools
import statistics

import numpy as np

from tests import resample_masked_ref as M

F = np.float32
U = np.uint64
MASK = U(0xFFFFFFFF)
M0, M1 = U(0xD2511F53), U(0xCD9E8D57)
W0, W1 = U(0x9E3779B9), U(0xBB67AE85)

# the published known-answer vectors of Philox4x32-10 (Random123's kat_vectors): (counter, key, result)
KAT = (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)))


def philox(c0, c1, c2, c3, k0, k1):
    """Four uint64 arrays of 32-bit words (the broadcast shape of the arguments): ten rounds, the key bumped between them."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=U) & MASK for c in (c0, c1, c2, c3)))
    k0, k1 = U(int(k0) & 0xFFFFFFFF), U(int(k1) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                       # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> U(32)) ^ c1 ^ k0, p1 & MASK, (p0 >> U(32)) ^ c3 ^ k1, p0 & MASK
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


@functools.lru_cache(maxsize=None)
def gauss_table():
    """65 536 fp32: gauss[u] = float32(inverse normal CDF((u + 0.5) / 65536)), the quantile computed in float64."""
    inv = statistics.NormalDist().inv_cdf
    return np.array([inv((u + 0.5) / 65536) for u in range(65536)], dtype=np.float64).astype(F)


def threshold(P):
    """T = floor(P * 2^32) as an integer (float64 arithmetic: exact for the product by a power of two)."""
    return int(np.floor(np.float64(P) * np.float64(4294967296.0)))


def words(B, p, key, step, first=0):
    """(w0, w1, w2, w3), each (B,1,p,p) uint64: counter (y * p + x, first + b, step, 0), key (lo, hi)."""
    c0 = np.arange(p * p, dtype=U).reshape(1, 1, p, p)
    c1 = (np.arange(B, dtype=U) + U(first)).reshape(B, 1, 1, 1)
    return philox(c0, c1, U(step), U(0), key[0], key[1])


def units(codes, levels):
    """A noise parameter given in codes, in value units: float32(float64(codes) / levels)."""
    return F(np.float64(codes) / levels)


def edges(lr, masked, edge_thr):
    """(B,1,p,p) bool: fabsf(v - n) > edge_thr for any 4-neighbour n inside the map (masked: a hole neighbour does not count)."""
    lr = np.asarray(lr, dtype=F)
    e = np.zeros(lr.shape, dtype=bool)
    thr = F(edge_thr)
    for ax, lo in ((2, True), (2, False), (3, True), (3, False)):
        n = np.roll(lr, 1 if lo else -1, axis=ax)
        inside = np.ones(lr.shape, dtype=bool)
        idx = [slice(None)] * 4
        idx[ax] = 0 if lo else -1
        inside[tuple(idx)] = False                      # the rolled-in value comes from the other border
        d = np.abs(lr - n)
        assert d.dtype == F
        ok = inside & ((n != 0) if masked else True)
        e |= ok & (d > thr)
    return e


def sensor(lr, masked, key, step, first, sigma, quad, edge_thr, p_drop, p_edge, levels, lut, with_parts=False):
    """lr (B,1,p,p) fp32 -> out of the same shape: codon_lr_sensor.  sigma, quad, edge_thr in value units (fp32)."""
    lr = np.ascontiguousarray(lr, dtype=F)
    B, _, p, q = lr.shape
    assert p == q
    w0, w1, _, _ = words(B, p, key, step, first)
    hole = (lr == 0) if masked else np.zeros(lr.shape, dtype=bool)
    e = edges(lr, masked, edge_thr)
    td, te = threshold(p_drop), threshold(p_edge)
    dropped = (w1 < (U(td) + np.where(e, U(te), U(0)))) & ~hole if masked else np.zeros(lr.shape, dtype=bool)
    g = gauss_table()[(w0 >> U(16)).astype(np.int64)]
    s = F(sigma) + F(quad) * (lr * lr)
    v = lr + s * g
    assert g.dtype == s.dtype == v.dtype == F
    if masked:
        out = np.where(hole | dropped, F(0), M.snap(v, levels, lut)).astype(F)
    else:
        out = v
    return (out, hole, dropped, e, g) if with_parts else out


# ---- test inputs (shared by tests/test_gpu_sensor.py and tools/host_check.py) ------------------------------------------

SIZES = (4, 7, 33)                 # the upsampler's minimum, a row shorter than a wavefront, no multiple of the block
BATCHES = (1, 5, 64)
LEVELS = (255, 1000, 65535)
HOLES = ("none", "pattern", "block")
STEPS = (0, 1, (1 << 31) + 12345)
FIRSTS = (0, 37)
KEY = (0x9E3779B9, 0x00C0FFEE)
# sigma, quad, edge_thr in value units; the probabilities
PARAMS = {"noise": dict(sigma=0.01), "quad": dict(quad=0.02), "dropout": dict(p_drop=0.2),
          "edge": dict(p_edge=0.6, edge_thr=0.6), "all": dict(sigma=0.004, quad=0.01, p_drop=0.1, p_edge=0.5, edge_thr=0.55)}


def input_map(B, p, kind, levels, masked, seed=0):
    """(B,1,p,p) fp32: M.plane on the code grid (masked) or anywhere in (0, 1] (unmasked: a 0.0 is a value like any other);
    "block": a block of holes that touches the top border and the left corner."""
    v = M.plane(B, p, p, "pattern" if kind == "pattern" else "none", seed=seed, levels=levels if masked else None)
    if kind == "block":
        v[:, :, :2, :(p + 1) // 2] = 0
    return v


def cases(B, p):
    """The launches of one (B, p): every level count, both modes, every parameter set the mode takes, every hole kind, the
    steps and first samples cycling through them."""
    k = 0
    for levels in LEVELS:
        for masked in (1, 0):
            for name, prm in PARAMS.items():
                if not masked and ("p_drop" in prm or "p_edge" in prm):
                    if name != "all":
                        continue                                        # refused: dropout needs the masked mode
                    prm = dict(prm, p_drop=0.0, p_edge=0.0)
                for kind in HOLES:
                    full = dict(dict(sigma=0.0, quad=0.0, edge_thr=0.0, p_drop=0.0, p_edge=0.0), **prm)
                    full.update({n: F(full[n]) for n in ("sigma", "quad", "edge_thr")})
                    yield dict(name=f"B {B} p {p} levels {levels} masked {masked} {name} {kind}", levels=levels, masked=masked,
                               kind=kind, step=STEPS[(k + k // 3) % 3], first=FIRSTS[(k // 2) % 2], seed=k, **full)
                    k += 1


def run_case(c, lr):
    """The restatement's output of one case of `cases` on the map `lr`."""
    _, lut = M.tables(8 if c["levels"] == 255 else 16, c["levels"])
    return sensor(lr, c["masked"], KEY, c["step"], c["first"], c["sigma"], c["quad"], c["edge_thr"], c["p_drop"], c["p_edge"],
                  c["levels"], lut)
