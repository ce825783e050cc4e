"""numpy restatement of the D4 self-ensemble (codon_amd/csrc/d4.hip, codon_amd.ensemble.self_ensemble) -- TEST
INFRASTRUCTURE.  The reference ships no self-ensemble, so this is the definition; the kernels must match it BIT FOR BIT.
tests/test_d4_cpu.py pins it: its views are train_data_ref.d4 on square crops, inverse-of-view is the identity, and the merge
of eight equal planes returns the plane's bits.

Planes are (B,1,H,W) arrays.  16-bit planes travel as their BITS (np.uint16) where only bits are copied (views); the merge takes
float32 arrays -- the caller upcasts, exactly, with `upcast`."""
import numpy as np

UPRIGHT = (0, 2, 4, 6)
TRANSPOSED = (1, 3, 5, 7)


def view(c, op):
    """The D4 op of train_data.hip on the last two axes of c: op&1 transpose, then op&2 flip rows, then op&4 flip columns."""
    if op & 1:
        c = np.swapaxes(c, -1, -2)
    if op & 2:
        c = c[..., ::-1, :]
    if op & 4:
        c = c[..., :, ::-1]
    return c


def inverse(o, op):
    """Undo op&4, then undo op&2, then transpose if op&1."""
    if op & 4:
        o = o[..., :, ::-1]
    if op & 2:
        o = o[..., ::-1, :]
    if op & 1:
        o = np.swapaxes(o, -1, -2)
    return o


def views(x):
    """(upright (4B,1,H,W), transposed (4B,1,W,H)) of x (B,1,H,W): view k of image b at index 4*b + (k >> 1) of its batch.
    Pure permutations: any dtype, bits copied."""
    x = np.asarray(x)
    B, _, H, W = x.shape
    up = np.empty((4 * B, 1, H, W), dtype=x.dtype)
    tr = np.empty((4 * B, 1, W, H), dtype=x.dtype)
    for b in range(B):
        for k in range(8):
            (tr if k & 1 else up)[4 * b + (k >> 1), 0] = view(x[b, 0], k)
    return up, tr


def upcast(a, dt):
    """Exact fp32 value of a plane held as float32 ("f32"), float16 ("f16") or bf16 BITS in np.uint16 ("bf16")."""
    a = np.asarray(a)
    if dt == "bf16":
        assert a.dtype == np.uint16
        return (a.astype(np.uint32) << np.uint32(16)).view(np.float32)
    assert a.dtype == {"f32": np.float32, "f16": np.float16}[dt]
    return a.astype(np.float32)


def merge(upright, transposed):
    """out[b] = 0.125f * (((u0+u1)+(u2+u3)) + ((u4+u5)+(u6+u7))), u_k the inverse of view k's output, fp32 throughout, every
    add rounded on its own, in this order.  upright (4B,1,H,W), transposed (4B,1,W,H), float32; returns (B,1,H,W) float32."""
    upright, transposed = np.asarray(upright), np.asarray(transposed)
    assert upright.dtype == transposed.dtype == np.float32
    n, _, H, W = upright.shape
    assert n % 4 == 0 and transposed.shape == (n, 1, W, H)
    out = np.empty((n // 4, 1, H, W), dtype=np.float32)
    for b in range(n // 4):
        u = [inverse((transposed if k & 1 else upright)[4 * b + (k >> 1), 0], k) for k in range(8)]
        s = ((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7]))
        assert s.dtype == np.float32
        out[b, 0] = np.float32(0.125) * s
    return out


def self_ensemble(model, x, y, dt):
    """The whole path with a numpy callable `model(a, b) -> array of a's shape and dtype`; x, y as `views` takes them, the
    model's outputs as `upcast(., dt)` takes them."""
    ux, tx = views(x)
    uy, ty = views(y)
    return merge(upcast(model(ux, uy), dt), upcast(model(tx, ty), dt))


# ---- test inputs (shared by tests/test_gpu_d4.py and tools/host_check.py) -------------------------------------------------

SHAPES = ((1, 5, 7), (1, 32, 32), (1, 33, 70), (3, 37, 53))       # B x H x W: below one 32 x 32 tile, exactly one, ragged, a batch
BITS = {"f32": np.uint32, "f16": np.uint16, "bf16": np.uint16}


def random_bits(shape, dt, seed):
    """(B,1,H,W) of seeded random BIT PATTERNS of the dtype's width -- NaNs of many payloads, infinities and subnormals among
    them -- with a quiet NaN, a signalling-NaN pattern and -0.0 planted at the corners.  The views only copy."""
    B, H, W = shape
    t = BITS[dt]
    g = np.random.default_rng(seed)
    a = g.integers(0, np.iinfo(t).max, size=(B, 1, H, W), endpoint=True, dtype=t)
    top = 8 * t().itemsize - 1
    nan_q = {"f32": 0x7FC00001, "f16": 0x7E01, "bf16": 0x7FC1}[dt]
    nan_s = {"f32": 0xFF800001, "f16": 0xFC01, "bf16": 0xFF81}[dt]
    a[:, 0, 0, 0], a[:, 0, 0, -1], a[:, 0, -1, 0], a[:, 0, -1, -1] = nan_q, nan_s, 1 << top, nan_q ^ 3
    return a


def merge_values(n, h, w, dt, seed):
    """(n,1,h,w) finite values of the dtype (float32 / float16 arrays, bf16 as uint16 bits): a mix of magnitudes around 1e-3,
    around 1 and around 300, of both signs, so that the order of the eight adds shows in the low bits of the fp32 sum -- with
    1e-3 and 1 alone it shows for fp32 values only: eight 11-bit (fp16) or 8-bit (bf16) significands spread over 2^11 add
    exactly in fp32 in any order; over 2^19 they do not."""
    g = np.random.default_rng(seed)
    v = g.uniform(0.5, 2.0, size=(n, 1, h, w)) * g.choice([1e-3, 1.0, 300.0], size=(n, 1, h, w))
    v = (v * np.where(g.uniform(size=(n, 1, h, w)) < 0.3, -1.0, 1.0)).astype(np.float32)
    if dt == "f32":
        return v
    if dt == "f16":
        return v.astype(np.float16)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)
