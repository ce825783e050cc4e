"""numpy restatement of the training-batch synthesis (codon_amd/csrc/train_data.hip, codon_amd.train.synthesize) -- TEST
INFRASTRUCTURE.  The reference's degradation script is not shipped, so this is the definition, unpinned against the
reference; the kernels must match it BIT FOR BIT, and tests/test_train_cpu.py checks its downsample against
torch.nn.functional.interpolate(mode="bicubic", antialias=True)."""
import numpy as np

from oracle import upsample_oracle


def lut():
    """io.to_input's value of every u8 code: float64 divide by 255, then float32."""
    return (np.arange(256) / 255).astype(np.float32)


def d4(c, op):
    """The D4 op of a square crop: op&1 transpose, then op&2 flip rows, then op&4 flip columns."""
    if op & 1:
        c = c.T
    if op & 2:
        c = c[::-1]
    if op & 4:
        c = c[:, ::-1]
    return c


def crops(pool, descs, P):
    """(t, y): (B,1,P,P) fp32 each; descs rows = (pool offset, H, W, y0, x0, op), guidance right behind the depth map."""
    pool = np.asarray(pool, dtype=np.uint8)
    tab = lut()
    t, y = [], []
    for off, h, w, y0, x0, op in np.asarray(descs, dtype=np.int64).tolist():
        dep = pool[off:off + h * w].reshape(h, w)
        gui = pool[off + h * w:off + 2 * h * w].reshape(h, w)
        t.append(tab[d4(dep[y0:y0 + P, x0:x0 + P], op)])
        y.append(tab[d4(gui[y0:y0 + P, x0:x0 + P], op)])
    return np.stack(t)[:, None], np.stack(y)[:, None]


def _cubic(x, a=-0.5):
    x = abs(x)
    if x < 1:
        return ((a + 2) * x - (a + 3)) * x * x + 1
    if x < 2:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def down_weights(n, s):
    """(n/s, 4s) fp32: PIL's BICUBIC reduce weights (fp64, renormalised over the taps inside [0, n), rounded once)."""
    tab = np.zeros((n // s, 4 * s))
    for o in range(n // s):
        centre = (o + 0.5) * s
        first = o * s - 3 * s // 2
        for k in range(4 * s):
            i = first + k
            tab[o, k] = _cubic((i + 0.5 - centre) / s) if 0 <= i < n else 0.0
        tab[o] /= tab[o].sum()
    return tab.astype(np.float32)


def downsample(hr, s):
    """(B,1,P,P) fp32 -> (B,1,P/s,P/s): horizontal pass, then vertical, each a sequential fp32 sum over the 4s taps."""
    hr = np.asarray(hr, dtype=np.float32)
    B, _, P, _ = hr.shape
    p = P // s
    w = down_weights(P, s)
    idx = np.clip(np.arange(p)[:, None] * s - 3 * s // 2 + np.arange(4 * s)[None, :], 0, P - 1)     # (p, 4s)
    h = np.zeros((B, P, p), dtype=np.float32)
    for k in range(4 * s):
        h = h + w[None, None, :, k] * hr[:, 0][:, :, idx[:, k]]
    out = np.zeros((B, p, p), dtype=np.float32)
    for k in range(4 * s):
        out = out + w[None, :, k, None] * h[:, idx[:, k], :]
    assert out.dtype == np.float32
    return out[:, None]


def quantize(x):
    v = np.clip(np.asarray(x, dtype=np.float32), np.float32(0), np.float32(1)) * np.float32(255)
    return lut()[np.rint(v).astype(np.int64)]


def synthesize(pool, descs, s, P):
    """(x, y, t) of codon_amd.train.synthesize."""
    t, y = crops(pool, descs, P)
    x = quantize(upsample_oracle.bicubic_upsample(downsample(t, s), s))
    return x, y, t
