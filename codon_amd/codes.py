"""Code planes: (h,w) or (B,h,w) depth codes, uint8 or u16 carried as int16 / uint16, code 0 a hole, `top` the code
of 1.0 -- what fill, guided fill, stretch, the baselines, register, clean and cloud all work on.  Everything about one that is
not a kernel wrapper lives here, once: the checked argument (Planes), the per-stream workspaces, the device tables, the two
argument validators, the host edges (numpy <-> tensor, the writer) and the pieces the tools' command lines are made of."""
from __future__ import annotations

import math
import os
import typing

import numpy as np
import torch

from . import _lib as L
from . import io, ops

CODES = "(h,w) or (B,h,w) uint8 codes, or u16 codes as int16 / uint16"


class Planes(typing.NamedTuple):
    """A checked code-plane argument: src is contiguous, B images of h x w, codes of `bits` bits, top the code of 1.0; fmt is
    the CODON_FILL_* of the codes and ptr src's address as ctypes takes it for a void* (an int: no c_void_p object is built),
    both held -- a wrapper's call is a few microseconds of host time"""
    src: torch.Tensor
    B: int
    h: int
    w: int
    bits: int
    top: int
    fmt: int
    ptr: int

    @property
    def dev(self):
        """src's device, with ops._dev's refusals (no CPU path, contiguous): asked where the wrappers always asked"""
        return ops._dev(self.src)

    def out(self, ho: int = None, wo: int = None) -> torch.Tensor:
        """An empty tensor of the argument's dtype and leading shape: its own planes, or planes of ho x wo"""
        if ho is None:
            return torch.empty_like(self.src)
        return torch.empty((*self.src.shape[:-2], ho, wo), dtype=self.src.dtype, device=self.src.device)


def code_planes(who: str, codes: torch.Tensor, depth_max, expects: str = CODES) -> Planes:
    """The Planes of (h,w) / (B,h,w) uint8, int16 or uint16 codes; refusals by name"""
    if codes.dim() not in (2, 3) or codes.dtype not in (torch.uint8, torch.int16, torch.uint16):
        raise RuntimeError(f"{who} expects {expects}")
    if codes.dtype == torch.uint8:
        if depth_max not in (None, 255):
            raise ValueError(f"{who}: depth_max {depth_max!r} with 8-bit codes")
        bits, top = 8, 255
    else:
        bits, top = 16, 65535 if depth_max is None else depth_max
    io.check_depth_max(top)
    src = codes.contiguous()
    h, w = src.shape[-2:]
    B = src.numel() // (h * w) if h * w else 0
    if B < 1:
        raise ValueError(f"{who}: an empty map {tuple(codes.shape)}")
    return Planes(src, B, h, w, bits, int(top), L.FILL_U8 if bits == 8 else L.FILL_U16, src.data_ptr())


_ws: dict = {}              # filler -> (guards.PerStream -> uint8 workspace of the (device, stream, thread), those made under a capture)


def workspace(who: str, query: str, dev, B: int, h: int, w: int, batched: bool = False):
    """Filler `who`'s workspace for B planes of h x w on dev's current stream, sized by the library's `query` (capture-safe:
    guards.PerStream); no two fillers share one.  `query` answers for one plane, or (batched) for all B.  Call it with
    `dev` current."""
    from .guards import PerStream
    need = getattr(L.load(), query)(B, h, w) if batched else B * getattr(L.load(), query)(h, w)
    if need == 0:
        raise ValueError(f"{who}: a {h}x{w} plane (1..4096 each way)")
    per_stream, held = _ws.setdefault(who, (PerStream(), []))
    return per_stream.get(dev, lambda capturing: torch.empty(need, dtype=torch.uint8, device=dev), need=need, hold=held)


_dev_tabs: dict = {}


def on_device(key, make, dev):
    """The cached copy on `dev` of the host table make() builds, under `key`"""
    k = (key, dev)
    t = _dev_tabs.get(k)
    if t is None:
        t = _dev_tabs[k] = torch.from_numpy(np.ascontiguousarray(make())).to(dev)
    return t


def _upsample():
    from . import upsample                          # the tables' makers live there, and upsample imports this module
    return upsample


def code_table(depth_bits: int, depth_max: int, dev):
    """(table, top) on `dev` for codes of depth_bits bits: value = table[code], and top is the code of 1.0 -- upsample.u8_lut and
    255, or upsample.lut16(depth_max) and depth_max."""
    if depth_bits == 16:
        top = int(depth_max)
        return on_device(("lut16", top), lambda: _upsample().lut16(top), dev), top       # made on a miss only
    return on_device("lut", lambda: _upsample().u8_lut(), dev), 255


# ---- the validators of an argument ------------------------------------------------------------------------------------------------

def positive(who: str, name: str, v, what: str, allow_bool: bool = True) -> float:
    """v as a float; anything but a finite positive number is refused by name"""
    try:
        f = float(v)
    except (TypeError, ValueError):
        f = float("nan")
    if not (f > 0.0 and math.isfinite(f)) or (isinstance(v, bool) and not allow_bool):
        raise ValueError(f"{who}: {name} {v!r} ({what})")
    return f


def integer(who: str, name: str, v, lo: int, hi, what: str) -> int:
    """v as an int; anything but an integer (no bool) in lo..hi (hi None: unbounded) is refused by name"""
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or v < lo or (hi is not None and v > hi):
        raise ValueError(f"{who}: {name} {v!r} ({what})")
    return int(v)


def rel_q16(who: str, rel) -> int:
    """Rq = rint(65536 rel) of a relative tolerance in [0, 1), at most 65535 (CL_MAX_REL, CD_MAX_REL of the tile headers)"""
    try:
        r = float(rel)
    except (TypeError, ValueError):
        r = float("nan")
    q = int(np.rint(65536.0 * r)) if math.isfinite(r) else -1
    if isinstance(rel, bool) or not (0.0 <= r < 1.0) or q > 65535:
        raise ValueError(f"{who}: tolerance_rel {rel!r} (a number in [0, 1), at most 65535 / 65536)")
    return q


# ---- the host edges ---------------------------------------------------------------------------------------------------------------

def codes_tensor(plane) -> torch.Tensor:
    """A host tensor of a writable, contiguous copy of a numpy code plane: uint8, or the bits of u16 codes as int16."""
    a = np.array(plane)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


def write_codes(path: str, codes: torch.Tensor):
    """One (h,w) plane of codes as a PNG of its own depth: 8-bit grey for uint8, 16-bit for u16 codes held as int16 / uint16"""
    a = codes.cpu().numpy()
    if a.dtype == np.uint8:
        io.write_gray(path, a)
    else:
        io.write_depth16(path, a.view(np.uint16))


# ---- the pieces of the tools' command lines (clean, register, cloud, undistort) -------------------------------------------------------

def add_depth_args(ap, depth_unit: float = None):
    """--depth-bits and --depth-max; with a default for it, --depth-unit too"""
    ap.add_argument("--depth-bits", type=int, default=8, choices=(8, 16))
    ap.add_argument("--depth-max", type=int, default=None, metavar="N", help="the largest code of a 16-bit data set (default 65535)")
    if depth_unit is not None:
        ap.add_argument("--depth-unit", type=float, default=depth_unit, metavar="M", help=f"metres per code (default {depth_unit})")


def depth_args_of(ap, a):
    """top, the largest code, of add_depth_args' flags (a.depth_max itself is what the wrappers take: None but for a 16-bit set
    that names one); refusals through ap.error, --depth-unit's where add_depth_args added the flag"""
    if a.depth_max is not None and a.depth_bits != 16:
        ap.error("--depth-max needs --depth-bits 16")
    if a.depth_max is not None and not 1 <= a.depth_max <= 65535:
        ap.error(f"--depth-max {a.depth_max} must be in [1, 65535]")
    if hasattr(a, "depth_unit") and not (a.depth_unit > 0.0 and math.isfinite(a.depth_unit)):
        ap.error(f"--depth-unit {a.depth_unit} must be positive")
    return 255 if a.depth_bits == 8 else 65535 if a.depth_max is None else a.depth_max


def require_dir(ap, flag: str, path):
    if not os.path.isdir(path):
        ap.error(f"--{flag} {path} is not a directory")


def require_gpu() -> torch.device:
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: codon_amd has no CPU fallback")
    return torch.device("cuda:0")


def depth_files(directory: str, depth_bits: int, top: int, dev):
    """(name, the file's codes on dev) for every depth map of a directory, in the order of the names"""
    for name in sorted(os.listdir(directory)):
        yield name, codes_tensor(io.read_depth_plane(os.path.join(directory, name), depth_bits, top)).to(dev)
