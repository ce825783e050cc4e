"""x4/x8/x16 bicubic upsample used by the synthetic-input generator (bench.py).  Host side computes
the per-phase Keys weights (fp64 -> fp32, once); the gather + arithmetic runs in upsample.hip."""
import ctypes as C
import functools
import statistics

import numpy as np
import torch

from . import _lib as L
from . import ops
from .codes import code_planes, code_table, on_device, positive, workspace
from .io import check_depth_max


def _keys(d, a=-0.75):
    d = abs(d)
    if d <= 1.0:
        return (a + 2.0) * d ** 3 - (a + 3.0) * d ** 2 + 1.0
    if d < 2.0:
        return a * d ** 3 - 5.0 * a * d ** 2 + 8.0 * a * d - 4.0 * a
    return 0.0


@functools.lru_cache(maxsize=None)
def phase_weights(scale: int) -> np.ndarray:
    """(scale, 4) fp32: weights of taps i0-1..i0+2 for output phase r = dst mod scale.
    frac t = ((2r + 1 - s) mod 2s) / 2s  (integer numerator, see upsample.hip)."""
    tab = np.zeros((scale, 4), dtype=np.float64)
    for r in range(scale):
        num = (2 * r + 1 - scale) % (2 * scale)
        t = num / (2.0 * scale)
        tab[r] = [_keys(1.0 + t), _keys(t), _keys(1.0 - t), _keys(2.0 - t)]
    return tab.astype(np.float32)


# ---- the host-side tables of the degradation and of the code planes -------------------------------------------------------

def u8_lut() -> np.ndarray:
    """256 fp32 values: io.to_input's conversion of every code (float64 divide by 255, then float32)."""
    return (np.arange(256, dtype=np.float64) / 255).astype(np.float32)


def lut16(depth_max: int = 65535) -> np.ndarray:
    """65 536 fp32 values: code c of a 16-bit depth map as float32(float64(c) / depth_max) -- u8_lut's conversion on the data
    set's own scale (lut16(65535)[257 * k] == u8_lut()[k] bit for bit).  Codes above depth_max are refused at load time; their
    entries exist only so that no u16 indexes out of the table."""
    check_depth_max(depth_max)
    return (np.arange(65536, dtype=np.float64) / depth_max).astype(np.float32)


@functools.lru_cache(maxsize=None)
def gauss_table() -> np.ndarray:
    """65 536 fp32 values: gauss[u] = float32(Phi^-1((u + 0.5) / 65536)), the quantile computed in float64 by the standard
    library -- the Gaussian of the sensor model, indexed by the top 16 bits of a Philox word.  The kernel and the
    numpy restatement read the same table: no logf or cosf can make them differ.  Exactly antisymmetric, strictly increasing,
    +-4.3249 at the ends, mean 0, standard deviation 0.99998986."""
    inv = statistics.NormalDist().inv_cdf
    return np.array([inv((u + 0.5) / 65536) for u in range(65536)], dtype=np.float64).astype(np.float32)


@functools.lru_cache(maxsize=None)
def down_weights(size: int, scale: int) -> np.ndarray:
    """(size/scale, 4*scale) fp32: row o weighs input taps i = o*scale - 3*scale/2 + k (PIL's BICUBIC reduce: Keys a = -0.5
    stretched by scale, centre (o + 0.5) * scale, tap weight k((i + 0.5 - centre) / scale); taps outside [0, size) get 0 and
    the rest are renormalised).  fp64, rounded once to fp32."""
    p, taps = size // scale, 4 * scale
    tab = np.zeros((p, taps), dtype=np.float64)
    for o in range(p):
        c = (o + 0.5) * scale
        for k in range(taps):
            i = o * scale - 3 * scale // 2 + k
            if 0 <= i < size:
                tab[o, k] = _keys((i + 0.5 - c) / scale, a=-0.5)
        tab[o] /= tab[o].sum()
    return tab.astype(np.float32)


def bicubic_upsample(lr: torch.Tensor, scale: int) -> torch.Tensor:
    lib = L.load()
    if lr.dim() != 4 or lr.shape[1] != 1 or lr.dtype != torch.float32:
        raise RuntimeError("bicubic_upsample expects a (B,1,h,w) fp32 tensor")
    dev = ops._dev(lr)
    B, _, h, w = lr.shape
    wt = torch.from_numpy(phase_weights(scale)).to(dev)
    out = torch.empty((B, 1, h * scale, w * scale), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.codon_bicubic_upsample(B, h, w, scale, C.c_void_p(lr.data_ptr()), C.c_void_p(wt.data_ptr()),
                                           C.c_void_p(out.data_ptr()), ops._stream(dev)), "bicubic_upsample")
    return out


def bicubic_upsample_masked(lr: torch.Tensor, scale: int):
    """(hr, valid): bicubic_upsample of a map in which 0.0 marks a hole, mask-normalised -- a pixel none of whose
    16 taps is a hole gets bicubic_upsample's bits, one whose valid taps weigh at least 0.5 the ratio of the two sums, any
    other is a hole again (0.0, valid 0).  valid: (B,1,h*scale,w*scale) uint8."""
    lib = L.load()
    if lr.dim() != 4 or lr.shape[1] != 1 or lr.dtype != torch.float32:
        raise RuntimeError("bicubic_upsample_masked expects a (B,1,h,w) fp32 tensor")
    lr = lr.contiguous()
    dev = ops._dev(lr)
    B, _, h, w = lr.shape
    wt = torch.from_numpy(phase_weights(scale)).to(dev)
    out = torch.empty((B, 1, h * scale, w * scale), dtype=torch.float32, device=dev)
    valid = torch.empty((B, 1, h * scale, w * scale), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.codon_bicubic_upsample_masked(B, h, w, scale, C.c_void_p(lr.data_ptr()), C.c_void_p(wt.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), C.c_void_p(valid.data_ptr()), ops._stream(dev)),
                "bicubic_upsample_masked")
    return out, valid


# ---- pull-push hole filling of low-resolution maps --------------------------------------------------------------

def _fill_launch(dev, B: int, h: int, w: int, src_ptr: int, fmt: int, tab, top: int, out_ptr: int):
    """codon_fill_holes on dev's current stream, with the per-stream workspace"""
    with ops._on(dev):
        ws = workspace("fill_holes", "codon_fill_holes_workspace_bytes", dev, B, h, w)
        L.check(L.load().codon_fill_holes(B, h, w, C.c_void_p(src_ptr), fmt, C.c_void_p(tab.data_ptr()) if tab is not None else None,
                                          top, C.c_void_p(out_ptr), C.c_void_p(ws.data_ptr()), ws.numel(), ops._stream(dev)),
                "fill_holes")


def fill_holes(codes: torch.Tensor, depth_max: int = None) -> torch.Tensor:
    """A low-resolution map with its holes filled by pull-push, a new tensor of the same shape and dtype; the
    argument is not modified.  codes: (h,w) or (B,h,w) uint8 codes, or the bits of u16 codes as int16 / uint16, code 0 a hole
    (depth_max: 255 for uint8, default 65535 otherwise) -- or a (B,1,h,w) float32 map on the code grid of depth_max (default 255:
    code_table's 8-bit table; else the 16-bit table of depth_max), 0.0 a hole, as train.synthesize(degrade_holes=True) holds it
    between its two bicubics.  Valid pixels come back bit for bit, a map without a valid pixel comes back unchanged, and a hole
    never takes a value above the largest valid code.  Integer arithmetic, bit-exact: tests/fill_ref.py.  One launch up to
    64 x 64, three beyond; no host synchronisation."""
    expects = "(h,w) / (B,h,w) uint8, int16 or uint16 codes, or a (B,1,h,w) float32 map"
    if codes.dtype == torch.float32:                # on the grid
        if codes.dim() != 4 or codes.shape[1] != 1:
            raise RuntimeError(f"fill_holes expects {expects}")
        bits, top = (8, 255) if depth_max is None else (16, depth_max)
        check_depth_max(top)
        src = codes.contiguous()
        B, _, h, w = src.shape
        if B * h * w == 0:
            raise ValueError(f"fill_holes: an empty map {tuple(codes.shape)}")
        dev = ops._dev(src)
        fmt, tab = L.FILL_F32, code_table(bits, top, dev)[0]
    else:
        p = code_planes("fill_holes", codes, depth_max, expects)
        src, B, h, w, top, fmt, tab, dev = p.src, p.B, p.h, p.w, p.top, p.fmt, None, p.dev
    out = torch.empty_like(src)
    _fill_launch(dev, B, h, w, src.data_ptr(), fmt, tab, int(top), out.data_ptr())
    return out


# ---- guidance-aware pull-push hole filling ---------------------------------------------------------------------

FILL_SIGMA = 10.0           # the default range sigma in guidance codes: the prototype's value, untuned


def check_fill_sigma(who: str, sigma) -> float:
    """sigma as a float; anything but a finite positive number is refused by name"""
    return positive(who, "fill_sigma", sigma, "a positive number of guidance codes")


@functools.lru_cache(maxsize=None)
def _range_table(sigma: float) -> np.ndarray:
    d = np.arange(256, dtype=np.float64)
    t = np.maximum(1.0, np.rint(256.0 * np.exp(-d * d / (2.0 * sigma * sigma)))).astype(np.uint16)
    t.setflags(write=False)
    return t


def range_table(sigma: float = FILL_SIGMA, device=None):
    """The range table of the guided hole filler: T[d] = max(1, rint(256 exp(-d^2 / (2 sigma^2)))) for the
    guidance differences d = 0 .. 255, float64 on the host -- a (256,) read-only numpy uint16 array, T[0] = 256, never rising,
    never below 1.  With `device` the cached copy on that device instead (the u16 bits as a (256,) int16 tensor)."""
    s = check_fill_sigma("range_table", sigma)
    if device is None:
        return _range_table(s)
    return on_device(("range", s), lambda: _range_table(s).view(np.int16).copy(), torch.device(device))


def _guided_args(who: str, codes, guide, scale, sigma, depth_max, _table):
    """The argument checks and the strided-guide rules the guided filler and the joint bilateral upsampler share ->
    (the codes' Planes, guide row bytes, guide image bytes, range table on the device)"""
    p = code_planes(who, codes, depth_max)
    src, B, h, w = p.src, p.B, p.h, p.w
    if scale not in (4, 8, 16):
        raise ValueError(f"{who}: scale {scale!r} (4, 8 or 16)")
    dev = p.dev
    if guide.dtype != torch.uint8 or guide.dim() != codes.dim() or guide.device != src.device:
        raise RuntimeError(f"{who} expects a uint8 guide on the codes' device, (H,W) for (h,w) codes and (B,H,W) for (B,h,w) codes")
    if guide.dim() == 3 and guide.shape[0] != B:
        raise ValueError(f"{who}: {guide.shape[0]} guidance images for {B} maps")
    if guide.shape[-2] < h * scale or guide.shape[-1] < w * scale:
        raise ValueError(f"{who}: a {guide.shape[-2]}x{guide.shape[-1]} guide, smaller than the {h * scale}x{w * scale} that a "
                         f"{h}x{w} map gives at x{scale}")
    if guide.stride(-1) != 1 and guide.shape[-1] > 1:
        raise ValueError(f"{who}: the guide needs unit stride along a row (stride {guide.stride(-1)})")
    row_bytes = guide.stride(-2) if guide.shape[-2] > 1 else max(guide.shape[-1], guide.stride(-2))
    image_bytes = guide.stride(0) if guide.dim() == 3 and B > 1 else 0
    if _table is None:
        table = range_table(sigma, dev)
    elif (not isinstance(_table, torch.Tensor) or _table.shape != (256,) or _table.dtype not in (torch.int16, torch.uint16)
          or _table.device != src.device or not _table.is_contiguous()):
        raise RuntimeError(f"{who}: _table must be a contiguous (256,) int16 / uint16 tensor on the codes' device")
    else:
        table = _table
    return p, row_bytes, image_bytes, table


def fill_holes_guided(codes: torch.Tensor, guide: torch.Tensor, scale: int, sigma: float = FILL_SIGMA, depth_max: int = None,
                      _table: torch.Tensor = None) -> torch.Tensor:
    """fill_holes with the guidance image's say: a hole weighs each of the plain filler's four parents by the
    range table of the difference between its own guidance and the guidance attached to the parent, so that a hole beside an
    occlusion edge is filled from its own side.  A new tensor of the codes' shape and dtype; no argument is modified.
    codes: (h,w) or (B,h,w) uint8 codes, or the bits of u16 codes as int16 / uint16, code 0 a hole (depth_max: 255 for uint8,
    default 65535 otherwise).  guide: (H,W) or (B,H,W) uint8 on the same device with H >= h * scale, W >= w * scale and unit
    stride along a row; its top-left (h * scale, w * scale) is read IN PLACE through its row and image strides (a plane of a
    training-pool record, the corner of a larger image).  scale: 4, 8 or 16.  sigma: of range_table, in guidance codes.
    A constant guide gives fill_holes' bits.  _table is for the tests alone (a constant table, which also gives fill_holes'
    bits): a (256,) int16 / uint16 device tensor used instead of range_table(sigma); its entries are NOT checked -- nothing
    reads the device here -- and an entry outside 1 .. 256 makes the output undefined (a 0 can zero a sum of weights, which
    the kernels divide by).  Valid pixels come back bit for bit, a map without a valid pixel comes back unchanged, and
    a hole never takes a value above the largest valid code.  Integer arithmetic, bit-exact: tests/guided_fill_ref.py.  One
    launch up to 64 x 64, three beyond; no host synchronisation."""
    who = "fill_holes_guided"
    p, row_bytes, image_bytes, table = _guided_args(who, codes, guide, scale, sigma, depth_max, _table)
    dev, out = p.src.device, p.out()              # the device _guided_args has checked
    P_ = C.c_void_p
    with ops._on(dev):
        ws = workspace(who, "codon_fill_guided_workspace_bytes", dev, p.B, p.h, p.w)
        L.check(L.load().codon_fill_holes_guided(p.B, p.h, p.w, p.ptr, p.fmt, p.top,
                                                 P_(guide.data_ptr()), row_bytes, image_bytes, scale, P_(table.data_ptr()),
                                                 P_(out.data_ptr()), P_(ws.data_ptr()), ws.numel(), ops._stream(dev)), who)
    return out


# ---- the classical baselines: joint bilateral and bicubic upsampling of code planes ---------------------------------

JBU_SIGMA_S = 1.0           # the default spatial sigma of the joint bilateral upsampler in LOW-RESOLUTION pixels: untuned


def check_jbu_sigma_s(who: str, sigma_s) -> float:
    """sigma_s as a float; anything but a finite positive number is refused by name"""
    return positive(who, "sigma_s", sigma_s, "a positive number of low-resolution pixels")


@functools.lru_cache(maxsize=None)
def _spatial_table(scale: int, sigma_s: float) -> np.ndarray:
    t = np.zeros((scale, 4), dtype=np.uint16)
    for ph in range(scale):
        num = (2 * ph + 1 - scale) % (2 * scale)          # phase_weights' fraction, over 2 * scale
        for k in range(4):
            d = abs(num - 2 * scale * (k - 1)) / (2.0 * scale)
            t[ph, k] = max(1.0, np.rint(256.0 * np.exp(-d * d / (2.0 * sigma_s * sigma_s))))
    t.setflags(write=False)
    return t


def spatial_table(scale: int, sigma_s: float = JBU_SIGMA_S, device=None):
    """The spatial table of the joint bilateral upsampler: S[ph][k] = max(1, rint(256 exp(-d^2 / (2 sigma_s^2))))
    for the output phase ph = 0 .. scale - 1 and the taps k = 0 .. 3 of the bicubic's footprint, d the tap's distance from the
    pixel in low-resolution pixels, float64 on the host -- a (scale, 4) read-only numpy uint16 array, every entry 1 .. 256.
    With `device` the cached copy on that device instead (the u16 bits as a (scale, 4) int16 tensor)."""
    if scale not in (4, 8, 16):
        raise ValueError(f"spatial_table: scale {scale!r} (4, 8 or 16)")
    s = check_jbu_sigma_s("spatial_table", sigma_s)
    if device is None:
        return _spatial_table(scale, s)
    return on_device(("spatial", scale, s), lambda: _spatial_table(scale, s).view(np.int16).copy(), torch.device(device))


def joint_bilateral_upsample(codes: torch.Tensor, guide: torch.Tensor, scale: int, sigma_s: float = JBU_SIGMA_S,
                             sigma_r: float = FILL_SIGMA, depth_max: int = None, _table: torch.Tensor = None) -> torch.Tensor:
    """Joint bilateral upsampling (Kopf et al. 2007), the classical guided baseline in the network's place: codes of
    shape (..., h * scale, w * scale) and the input's dtype, no argument modified.  A high-resolution pixel takes the weighted
    mean of the valid codes in the bicubic's own 4 x 4 footprint, a tap weighing spatial_table(scale, sigma_s) of its distance
    times range_table(sigma_r) of the difference between the pixel's guidance and the tap's (the box mean of the guidance over
    the low-resolution pixel); a hole (code 0) weighs nothing, and the output is a hole exactly where the footprint holds no
    valid code.  codes, guide, scale, depth_max and _table (for the tests alone: the range table, unchecked) as
    fill_holes_guided takes them, the guide read IN PLACE through its strides.  sigma_s: in low-resolution pixels; sigma_r: in
    guidance codes.  Integer arithmetic, bit-exact: tests/jbu_ref.py.  Two launches; no host synchronisation."""
    who = "joint_bilateral_upsample"
    p, row_bytes, image_bytes, table = _guided_args(who, codes, guide, scale, sigma_r, depth_max, _table)
    dev = p.src.device                            # the device _guided_args has checked
    stab = spatial_table(scale, check_jbu_sigma_s(who, sigma_s), dev)
    out = p.out(p.h * scale, p.w * scale)
    P_ = C.c_void_p
    with ops._on(dev):
        ws = workspace(who, "codon_jbu_workspace_bytes", dev, p.B, p.h, p.w)
        L.check(L.load().codon_jbu_upsample(p.B, p.h, p.w, p.ptr, p.fmt, p.top,
                                            P_(guide.data_ptr()), row_bytes, image_bytes, scale, P_(table.data_ptr()),
                                            P_(stab.data_ptr()), P_(out.data_ptr()), P_(ws.data_ptr()), ws.numel(),
                                            ops._stream(dev)), who)
    return out


def bicubic_upsample_codes(codes: torch.Tensor, scale: int, depth_max: int = None) -> torch.Tensor:
    """The bicubic baseline: the hole-aware bicubic of codes_to_input, written as the INTEGER that function
    looks up before its cast, rint(clamp(up) * top) -- codes of shape (..., h * scale, w * scale) and the input's dtype, a hole
    of the rule staying 0.  (Not the float input truncated back: float32(k / 255) * 255 truncates to k - 1 for some k.)  codes:
    (h,w) or (B,h,w) uint8 codes, or the bits of u16 codes as int16 / uint16 (depth_max: default 65535).  One launch."""
    return _lr_codes("bicubic_upsample_codes", "codon_lr_codes_upsample", "bicubic_upsample_codes", codes, scale, depth_max)


def codes_to_input(codes: torch.Tensor, scale: int, tdt, depth_max: int = None) -> torch.Tensor:
    """The network's depth input from a low-resolution code plane on the device, ONE launch (codon_lr_codes_to_input):
    codes (h,w) or (B,h,w), uint8 (value = code / 255) or the bits of u16 codes as int16 / uint16 (value = code / depth_max,
    default 65535), code 0 a hole -> the mask-normalised bicubic x`scale` (bicubic_upsample_masked) -> back onto the
    code grid -> tdt, as (B,1,h*scale,w*scale).  Bit for bit what train.synthesize(degrade_holes=True) builds from the same
    low-resolution values."""
    return _lr_codes("codes_to_input", "codon_lr_codes_to_input", "lr_codes_to_input", codes, scale, depth_max, tdt)


def _lr_codes(who: str, entry: str, label: str, codes, scale, depth_max, tdt=None):
    """The one body of the two: the hole-aware bicubic x`scale` of a code plane through `entry` -- codes of the argument's dtype
    and leading shape, or with tdt the (B,1,H,W) input of that dtype"""
    p = code_planes(who, codes, depth_max)
    if scale not in (4, 8, 16):
        raise ValueError(f"{who}: scale {scale!r} (4, 8 or 16)")
    if tdt is not None and tdt not in ops.DTYPE_CODE:
        raise ValueError(f"{who}: dtype {tdt!r} (float32, float16 or bfloat16)")
    dev = p.dev
    lut, top = code_table(p.bits, p.top, dev)
    wt = on_device(("up", scale), lambda: phase_weights(scale), dev)
    H, W = p.h * scale, p.w * scale
    out = p.out(H, W) if tdt is None else torch.empty((p.B, 1, H, W), dtype=tdt, device=dev)
    with ops._on(dev):                                # addresses as ints: ctypes takes them for a void*
        L.check(getattr(L.load(), entry)(p.B, p.h, p.w, scale, p.ptr, p.bits, lut.data_ptr(), top, wt.data_ptr(), out.data_ptr(),
                                         *(() if tdt is None else (ops.DTYPE_CODE[tdt],)), ops._stream(dev)), label)
    return out


# ---- per-image range normalisation of depth codes --------------------------------------------------------------

def check_stretch_top(who: str, depth_max: int):
    """The stretch maps onto [1, depth_max] with depth_max - 1 steps: a grid of fewer than two codes is refused by name."""
    if depth_max < 2:
        raise ValueError(f"{who}: depth_max {depth_max!r} leaves per-image normalisation no grid to stretch onto (at least 2)")


def code_range(codes: torch.Tensor) -> torch.Tensor:
    """(B, 2) int32 on the codes' device: per image (lo, hi), the smallest non-zero and the largest code of the plane, (0, 0)
    for a plane without a valid code.  codes: (h,w) or (B,h,w) uint8 codes, or the bits of u16 codes as
    int16 / uint16, code 0 a hole.  One launch, one workgroup per image; nothing is read back."""
    p = code_planes("code_range", codes, None)
    dev = p.dev
    lo_hi = torch.empty((p.B, 2), dtype=torch.int32, device=dev)
    with ops._on(dev):
        L.check(L.load().codon_code_range(p.B, p.h, p.w, p.ptr, p.bits, lo_hi.data_ptr(), ops._stream(dev)), "code_range")
    return lo_hi


def _map_codes(who: str, entry: str, codes, lo_hi, depth_max, out):
    p = code_planes(who, codes, depth_max)
    check_stretch_top(who, p.top)
    dev = p.dev
    if lo_hi is None:
        lo_hi = code_range(p.src)
    else:
        lo_hi = torch.as_tensor(lo_hi, dtype=torch.int32, device=dev).reshape(-1, 2).contiguous()
        if lo_hi.shape[0] != p.B:
            raise ValueError(f"{who}: {lo_hi.shape[0]} ranges for {p.B} images")
    if out is None:
        out = p.out()
    elif out.shape != codes.shape or out.dtype != codes.dtype or out.device != p.src.device or not out.is_contiguous():
        raise ValueError(f"{who}: out must be a contiguous tensor of the codes' shape, dtype and device")
    with ops._on(dev):
        L.check(getattr(L.load(), entry)(p.B, p.h, p.w, p.ptr, p.bits, p.top, lo_hi.data_ptr(), out.data_ptr(), ops._stream(dev)), who)
    return out, lo_hi


def stretch_codes(codes: torch.Tensor, depth_max: int = None, lo_hi: torch.Tensor = None, out: torch.Tensor = None):
    """(codes', lo_hi): every image's valid codes [lo, hi] stretched onto [1, top] of the data's own grid -- top 255 for uint8
    codes, depth_max (default 65535) for u16 codes held as int16 / uint16 -- code 0, a hole, staying 0:
    c' = 1 + (2 (clamp(c, lo, hi) - lo) (top - 1) + n) // (2 n) with n = hi - lo, top when n == 0, in integers, bit-exact
    (tests/stretch_ref.py).  codes: (h,w) or (B,h,w); a new tensor of the same shape and dtype comes back and the argument is
    not modified, unless `out` names the result's tensor, which may be `codes` itself.  lo_hi: (B, 2) int32 on the device --
    code_range(codes) when None (one more launch); another plane's range clamps the codes into it.  A plane without a valid
    code, range (0, 0), comes back as it is.  No host synchronisation."""
    return _map_codes("stretch_codes", "codon_stretch_codes", codes, lo_hi, depth_max, out)


def unstretch_codes(codes: torch.Tensor, lo_hi: torch.Tensor, depth_max: int = None, out: torch.Tensor = None) -> torch.Tensor:
    """stretch_codes undone on codes of the stretched grid (the network's output after post-processing):
    o = lo + (2 (max(o', 1) - 1) n + top - 1) // (2 (top - 1)), a value in [lo, hi]; unstretch_codes(*stretch_codes(c)) == c
    bit for bit on valid codes.  lo_hi: the (B, 2) int32 device tensor stretch_codes returned.  One launch, no host
    synchronisation."""
    if lo_hi is None:
        raise ValueError("unstretch_codes: lo_hi is needed (the range stretch_codes returned)")
    return _map_codes("unstretch_codes", "codon_unstretch_codes", codes, lo_hi, depth_max, out)[0]
