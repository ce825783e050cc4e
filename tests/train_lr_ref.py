"""numpy restatement of training on real low-resolution depth maps (train_crops_lr_kernel in
codon_amd/csrc/resample_masked.hip, codon_amd.train.synthesize on a TrainSet(lr_dir=...)) -- TEST INFRASTRUCTURE.  There is no
reference for it; the kernel must match this BIT FOR BIT.

    x = D4(quantize(upsample_masked(lut[codes]))[window]),   t = D4(lut[depth][window]),   y = D4(lut8[guidance][window])

Everything numeric comes from the existing restatements, used unchanged: tests/resample_masked_ref.py (the hole-aware upsample
of the WHOLE low-resolution plane and the quantisation onto the code grid), tests/train_data_ref.py (the D4 op, the u8 table)
and tests/train_data16_ref.py (lut16).  What is stated here is the record layout and the order: upsample the whole plane,
THEN take the window -- the border clamp is the image's, and y0 / x0 need not be multiples of the scale."""
import os

import numpy as np

from tests import resample_masked_ref as M
from tests import train_data_ref as R

F = np.float32


def pack(records, depth_bits):
    """The byte pool of [(depth (H,W), guide u8 (H,W), lr codes (h,w)), ...] and every record's byte offset.
    8 bits:  depth u8, guidance u8, LR codes u8.
    16 bits: depth little-endian u16, LR codes u16, guidance u8; the next record starts at the next even offset."""
    out, offsets = bytearray(), []
    for depth, guide, lr in records:
        offsets.append(len(out))
        if depth_bits == 8:
            for p in (depth, guide, lr):
                out += np.ascontiguousarray(p).astype(np.uint8).tobytes()
        else:
            out += np.ascontiguousarray(depth).astype("<u2").tobytes()
            out += np.ascontiguousarray(lr).astype("<u2").tobytes()
            out += np.ascontiguousarray(guide).astype(np.uint8).tobytes()
            if len(out) % 2:
                out += b"\0"
    return np.frombuffer(bytes(out), dtype=np.uint8), offsets


def planes(pool, off, H, W, s, depth_bits):
    """(depth, guide, lr codes) of the record at byte offset off; (H, W) the HR size, the LR plane (H/s, W/s)."""
    pool = np.asarray(pool, dtype=np.uint8)
    assert H % s == 0 and W % s == 0
    n, h, w = H * W, H // s, W // s
    if depth_bits == 8:
        return (pool[off:off + n].reshape(H, W), pool[off + n:off + 2 * n].reshape(H, W),
                pool[off + 2 * n:off + 2 * n + h * w].reshape(h, w))
    assert off % 2 == 0
    k = off + 2 * n
    return (pool[off:k].view("<u2").reshape(H, W), pool[k + 2 * h * w:k + 2 * h * w + n].reshape(H, W),
            pool[k:k + 2 * h * w].view("<u2").reshape(h, w))


def whole_input(codes, s, levels, lut):
    """(x (H,W) fp32, branch (H,W)) of one whole LR code plane (h,w): what inference builds from the file, in fp32, and which
    branch of the rule every HR pixel took."""
    v = np.asarray(lut, dtype=F)[np.asarray(codes).astype(np.int64)][None, None]
    up, _, branch = M.upsample_masked(v, s, with_branch=True)
    return M.quantize(up, levels, lut)[0, 0], branch[0, 0]


def synthesize(pool, descs, s, P, depth_bits, depth_max=65535, with_branch=False):
    """(x, y, t) of codon_amd.train.synthesize on a TrainSet with low-resolution maps: (B,1,P,P) fp32 each; descs rows =
    (pool offset, H, W, y0, x0, op).  with_branch: (x, y, t, branch), the rule's branch of every x."""
    levels, lut = M.tables(depth_bits, depth_max)
    lut8 = R.lut()
    whole = {}
    x, y, t, br = [], [], [], []
    for off, H, W, y0, x0, op in np.asarray(descs, dtype=np.int64).tolist():
        depth, guide, lr = planes(pool, off, H, W, s, depth_bits)
        if off not in whole:
            whole[off] = whole_input(lr, s, levels, lut)
        full, branch = whole[off]
        win = (slice(y0, y0 + P), slice(x0, x0 + P))
        x.append(R.d4(full[win], op))
        br.append(R.d4(branch[win], op))
        y.append(lut8[R.d4(guide[win], op)])
        t.append(lut[R.d4(depth[win], op).astype(np.int64)])
    out = tuple(np.ascontiguousarray(np.stack(a)[:, None]) for a in (x, y, t))
    return out + (np.stack(br)[:, None],) if with_branch else out


def codes_of(v, levels):
    """The codes of values on the code grid (resample_masked_ref.plane(levels=...)): lut[code] == v."""
    return np.rint(np.asarray(v, dtype=np.float64) * levels).astype(np.uint16 if levels > 255 else np.uint8)


def windows(H, W, P):
    """The five windows of the tests: the four corners and an interior one that no scale aligns."""
    return [(0, 0), (H - P, W - P), (0, W - P), (H - P, 0), ((H - P) // 2 + 1, (W - P) // 2 + 3)]


# ---- the cases of the tests ---------------------------------------------------------------------------------------------------

CROPS = {4: 16, 8: 32, 16: 64}


def records(lrs, s, levels, seed=0):
    """[(depth, guide, lr codes)] for LR code planes `lrs`: random HR depth codes 0 .. levels (about 5 % holes, the extremes
    present) and random guidance of the size each LR plane fixes."""
    g = np.random.default_rng(7000 + seed)
    out = []
    for lr in lrs:
        H, W = lr.shape[0] * s, lr.shape[1] * s
        depth = g.integers(1, levels + 1, size=(H, W)).astype(lr.dtype)
        depth[g.uniform(size=(H, W)) < 0.05] = 0
        depth.reshape(-1)[:3] = [0, 1, levels]
        out.append((depth, g.integers(0, 256, size=(H, W), dtype=np.uint8), lr))
    return out


def case(s, levels, kind="pattern", shapes=((9, 13),) * 3, seed=None):
    """(records, rows) with rows = (image, H, W, y0, x0, op): one LR plane per entry of `shapes` (equal shapes come from ONE
    resample_masked_ref.plane call, seed = the scale unless given), every image's five windows at crop CROPS[s], the eight D4
    ops cycling over the windows."""
    seed = s if seed is None else seed
    P = CROPS[s]
    lrs, k = [], 0
    while k < len(shapes):
        n = 1
        while k + n < len(shapes) and shapes[k + n] == shapes[k]:
            n += 1
        v = M.plane(n, shapes[k][0], shapes[k][1], kind, seed=seed + k, levels=levels)
        lrs += [codes_of(v[b, 0], levels) for b in range(n)]
        k += n
    recs = records(lrs, s, levels, seed)
    rows = []
    for i, lr in enumerate(lrs):
        H, W = lr.shape[0] * s, lr.shape[1] * s
        for y0, x0 in windows(H, W, P):
            rows.append([i, H, W, y0, x0, len(rows) % 8])
    return recs, rows


def descs_of(rows, offsets):
    """rows (image, H, W, y0, x0, op) -> descriptor rows (pool offset, H, W, y0, x0, op)."""
    return np.asarray([[offsets[i], H, W, y0, x0, op] for i, H, W, y0, x0, op in rows], dtype=np.int64)


def write_set(root, recs, depth_bits, extra=(0, 0, 0, 0)):
    """depth/, color/, lr/ under root, one PNG per record (16-bit depth and LR files at 16 bits); depth map and guidance padded
    by `extra` = (depth rows, depth cols, guidance rows, guidance cols) beyond the size the LR plane fixes."""
    from codon_amd import io
    dirs = [os.path.join(root, n) for n in ("depth", "color", "lr")]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    deep = io.write_depth16 if depth_bits == 16 else io.write_gray
    for i, (depth, guide, lr) in enumerate(recs):
        deep(os.path.join(dirs[0], f"{i:02d}.png"), np.pad(depth, ((0, extra[0]), (0, extra[1])), mode="edge"))
        io.write_gray(os.path.join(dirs[1], f"{i:02d}.png"), np.pad(guide, ((0, extra[2]), (0, extra[3])), mode="edge"))
        deep(os.path.join(dirs[2], f"{i:02d}.png"), lr)
    return dirs
