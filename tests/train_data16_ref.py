"""numpy restatement of the 16-bit depth path -- TEST INFRASTRUCTURE, written from the definitions and
independent of the kernels: the record layout of the byte pool, the D4 op, lut16, the quantisation onto the data set's code
grid, the post-processing to u16 codes and the masked squared error.  There is no reference for any of it (the reference's
data is 8-bit); the kernels must match this BIT FOR BIT.  The table of the guidance, the D4 op, the downsample and the
upsample are those of tests/train_data_ref.py and oracle/upsample_oracle.py, used unchanged."""
import os

import numpy as np

from oracle import upsample_oracle
from tests import train_data_ref as R


def lut16(depth_max=65535):
    """code c -> float32(float64(c) / depth_max), for every u16."""
    return (np.arange(65536, dtype=np.float64) / depth_max).astype(np.float32)


def pack(records):
    """The byte pool of [(depth u16 (H,W), label u16 (H,W) or None, guide u8 (H,W)), ...] and the byte offset of every record:
    depth plane (little-endian u16), label plane if any, guidance bytes; the next record starts at the next even offset."""
    out, offsets = bytearray(), []
    for depth, label, guide in records:
        offsets.append(len(out))
        out += np.ascontiguousarray(depth).astype("<u2").tobytes()
        if label is not None:
            out += np.ascontiguousarray(label).astype("<u2").tobytes()
        out += np.ascontiguousarray(guide).astype(np.uint8).tobytes()
        if len(out) % 2:
            out += b"\0"
    return np.frombuffer(bytes(out), dtype=np.uint8), offsets


def planes(pool, off, h, w, labeled):
    """(depth, label or None, guide) of the record at byte offset off."""
    pool = np.asarray(pool, dtype=np.uint8)
    n = h * w
    depth = pool[off:off + 2 * n].view("<u2").reshape(h, w)
    k = off + 2 * n
    label = None
    if labeled:
        label = pool[k:k + 2 * n].view("<u2").reshape(h, w)
        k += 2 * n
    return depth, label, pool[k:k + n].reshape(h, w)


def crops(pool, descs, P, depth_max, labeled):
    """(source, y, t): (B,1,P,P) fp32 each; t is source itself without a label plane."""
    tab16, tab8 = lut16(depth_max), R.lut()
    src, y, t = [], [], []
    for off, h, w, y0, x0, op in np.asarray(descs, dtype=np.int64).tolist():
        assert off % 2 == 0
        depth, label, guide = planes(pool, off, h, w, labeled)
        win = (slice(y0, y0 + P), slice(x0, x0 + P))
        src.append(tab16[R.d4(depth[win], op)])
        y.append(tab8[R.d4(guide[win], op)])
        t.append(tab16[R.d4(label[win], op)] if labeled else src[-1])
    return tuple(np.stack(a)[:, None] for a in (src, y, t))


def quantize(x, depth_max):
    """lut16[rint(clamp(x, 0, 1) * float32(depth_max))]: fp32 product, round half to even.  (No NaN here: numpy's clip keeps
    it, the kernel's fmaxf turns it into 0 -- the tests state that rule themselves.)"""
    v = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(depth_max)
    assert v.dtype == np.float32
    return lut16(depth_max)[np.rint(v).astype(np.int64)]


def synthesize(pool, descs, s, P, depth_max, labeled):
    """(x, y, t) of codon_amd.train.synthesize on a 16-bit TrainSet."""
    src, y, t = crops(pool, descs, P, depth_max, labeled)
    x = quantize(upsample_oracle.bicubic_upsample(R.downsample(src, s), s), depth_max)
    return x, y, t


def postprocess_u16(x, depth_max):
    """x: float32 / float16 numpy array, or the uint16 BIT PATTERNS of bf16 values (numpy has no bf16).  Upcast to fp32
    (exact), clamp, times float32(depth_max) in fp32, rint (half to even); NaN -> 0."""
    x = np.asarray(x)
    if x.dtype == np.uint16:
        x = (x.astype(np.uint32) << 16).view(np.float32)
    x = x.astype(np.float32)
    x = np.where(np.isnan(x), np.float32(0), x)
    v = np.clip(x, np.float32(0), np.float32(1)) * np.float32(depth_max)
    assert v.dtype == np.float32
    return np.rint(v).astype(np.uint16)


def masked_sqerr(label_u16, out_u16):
    """(sum of squared code differences, count) over label != 0 as Python integers, from int64."""
    lab = np.asarray(label_u16).astype(np.int64)[:out_u16.shape[0], :out_u16.shape[1]]
    d = lab - np.asarray(out_u16).astype(np.int64)
    v = lab != 0
    return int((d[v] * d[v]).sum()), int(v.sum())


def _io():
    from codon_amd import io
    return io


def write_set(root, sizes, label=True, seed=0, depth_max=65535):
    """depth/, color/ (8-bit, one pixel larger), label/ (16-bit with holes): three planes of different content."""
    g = np.random.default_rng(seed)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "label")]
    for d in dirs[:3 if label else 2]:
        os.makedirs(d, exist_ok=True)
    recs = []
    for i, (h, w) in enumerate(sizes):
        dep = g.integers(1, depth_max + 1, size=(h, w)).astype(np.uint16)
        dep.reshape(-1)[:3] = [0, 1, depth_max]
        gui = g.integers(0, 256, size=(h + 1, w + 1), dtype=np.uint8)
        lab = g.integers(1, depth_max + 1, size=(h, w)).astype(np.uint16)
        lab[g.uniform(size=(h, w)) < 0.1] = 0
        lab.reshape(-1)[-3:] = [depth_max, 1, 0]
        _io().write_depth16(os.path.join(dirs[0], f"{i:02d}.png"), dep)
        _io().write_gray(os.path.join(dirs[1], f"{i:02d}.png"), gui)
        if label:
            _io().write_depth16(os.path.join(dirs[2], f"{i:02d}.png"), lab)
        recs.append((dep, lab if label else None, gui[:h, :w]))
    return dirs[0], dirs[1], (dirs[2] if label else None), recs
