"""Outlier rejection of a depth sensor's maps: flying pixels -- the mixed measurements a time-of-flight or
structured-light camera writes at an occlusion edge, between the two surfaces -- and speckles, the small islands of depth inside
its shadow regions, become code 0.  Nothing else changes: every output code is the input code or 0.  It runs in the SENSOR's own
frame, before `python -m codon_amd.register` (which has --clean for the same step on one upload): after the projection an
outlier's neighbours are other pixels.

    python -m codon_amd.clean --depth DIR --out DIR [--depth-bits {8,16}] [--depth-max N] [--tolerance CODES] [--tolerance-rel F]
                              [--min-support K] [--min-region N] [--stats]

The definition, in integers (tests/clean_ref.py; csrc/clean.hip): two pixels are linked when both are valid and their codes
differ by at most tolerance + tolerance_rel * the smaller code.  Rule 1: a valid pixel with fewer than --min-support linked
pixels among its 8 neighbours inside the plane is removed; one pass over the input, not idempotent; 0 switches it off; above 3
it removes the image's corners, above 5 its border.  Rule 2: a connected component (4-connectivity, neighbours in one component
when linked) of fewer than --min-region pixels of what rule 1 left is removed; 0 or 1 switches it off.  The four defaults are
untuned.  Not handled: a real structure one pixel wide (a wire) goes with the flying pixels; no confidence or amplitude image is
read; nothing is filtered over time."""
from __future__ import annotations

import argparse
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import io, ops
from .upsample import _code_planes, _workspace

MAX_SUPPORT, MAX_REGION, MAX_REL_Q16 = 8, 1 << 24, 65535
STATS = ("valid", "flying", "speckle", "regions")
DEFAULTS = dict(tolerance=2, tolerance_rel=0.02, min_support=3, min_region=16)


def _integer(who: str, name: str, v, lo: int, hi: int, what: str) -> int:
    if not isinstance(v, (int, np.integer)) or isinstance(v, bool) or not lo <= v <= hi:
        raise ValueError(f"{who}: {name} {v!r} ({what})")
    return int(v)


def rel_q16(who: str, rel) -> int:
    """Rq = rint(65536 rel) of a relative tolerance in [0, 1), at most 65535"""
    try:
        r = float(rel)
    except (TypeError, ValueError):
        r = float("nan")
    q = int(np.rint(65536.0 * r)) if math.isfinite(r) else -1
    if isinstance(rel, bool) or not (0.0 <= r < 1.0) or q > MAX_REL_Q16:
        raise ValueError(f"{who}: tolerance_rel {rel!r} (a number in [0, 1), at most 65535 / 65536)")
    return q


class Cleaner:
    """clean(codes) removes flying pixels and speckles from a batch of the depth camera's own planes.  tolerance: codes;
    tolerance_rel: a fraction of the smaller code; min_support: K of rule 1 (0: off); min_region: N of rule 2 (0, 1: off)."""

    def __init__(self, tolerance: int = 2, tolerance_rel: float = 0.02, min_support: int = 3, min_region: int = 16):
        who = "Cleaner"
        self.tolerance = _integer(who, "tolerance", tolerance, 0, 65535, "an integer number of codes, 0 .. the largest code")
        self.tolerance_rel = tolerance_rel
        self.tolerance_rel_q16 = rel_q16(who, tolerance_rel)
        self.min_support = _integer(who, "min_support", min_support, 0, MAX_SUPPORT, f"an integer in 0..{MAX_SUPPORT}")
        self.min_region = _integer(who, "min_region", min_region, 0, MAX_REGION, f"an integer in 0..{MAX_REGION}")

    def __call__(self, codes: torch.Tensor, depth_max: int = None, stats: bool = False):
        """codes: (h, w) or (B, h, w) uint8 codes, or u16 codes as int16 / uint16 (read as unsigned), 0 a hole, on a GPU -> codes
        of the argument's shape and dtype, each the argument's code or 0; the argument is not modified.  stats=True: (codes,
        int32 (B, 4) on the device: valid inputs, pixels removed by rule 1, pixels removed by rule 2, components removed by
        rule 2).  Two launches with rule 2 off, four with it on; no host synchronisation."""
        who = "clean_depth"
        src, B, h, w, bits, top = _code_planes(who, codes, depth_max)
        if self.tolerance > top:
            raise ValueError(f"{who}: tolerance {self.tolerance} above the largest code {top}")
        dev = ops._dev(src)
        out = torch.empty_like(src)
        counts = torch.empty((B, 4), dtype=torch.int32, device=dev) if stats else None
        P_ = C.c_void_p
        with torch.cuda.device(dev):
            ws = _workspace(who, "codon_clean_workspace_bytes", dev, B, h, w, batched=True)
            L.check(L.load().codon_clean_depth(B, h, w, P_(src.data_ptr()), L.FILL_U8 if bits == 8 else L.FILL_U16, top, self.tolerance,
                                               self.tolerance_rel_q16, self.min_support, self.min_region, P_(out.data_ptr()),
                                               P_(counts.data_ptr()) if stats else None, P_(ws.data_ptr()), ws.numel(),
                                               ops._stream(dev)), who)
        return (out, counts) if stats else out


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def add_arguments(ap, prefix: str = ""):
    """--tolerance, --tolerance-rel, --min-support, --min-region under `prefix` ("clean-" for register's)"""
    ap.add_argument(f"--{prefix}tolerance", type=int, default=DEFAULTS["tolerance"], metavar="CODES",
                    help="two pixels are linked when their codes differ by at most this ... (default 2, untuned)")
    ap.add_argument(f"--{prefix}tolerance-rel", type=float, default=DEFAULTS["tolerance_rel"], metavar="F",
                    help="... plus this fraction of the smaller code (default 0.02, untuned)")
    ap.add_argument(f"--{prefix}min-support", type=int, default=DEFAULTS["min_support"], metavar="K",
                    help="a pixel with fewer linked pixels among its 8 neighbours is a flying pixel; 0: off (default 3, untuned)")
    ap.add_argument(f"--{prefix}min-region", type=int, default=DEFAULTS["min_region"], metavar="N",
                    help="a connected component of fewer pixels is a speckle; 0, 1: off (default 16, untuned)")


def cleaner_of(a, ap, prefix: str = "") -> Cleaner:
    """The Cleaner of parsed arguments; what it refuses is the parser's error"""
    get = lambda n: getattr(a, (prefix + n).replace("-", "_"))            # noqa: E731
    try:
        return Cleaner(get("tolerance"), get("tolerance-rel"), get("min-support"), get("min-region"))
    except ValueError as e:
        ap.error(str(e).replace("Cleaner: ", "--" + prefix).replace("_", "-"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m codon_amd.clean", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", required=True, metavar="DIR", help="the sensor's depth maps, in the depth camera's own frame")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the cleaned maps go, under the same file names")
    ap.add_argument("--depth-bits", type=int, default=8, choices=(8, 16))
    ap.add_argument("--depth-max", type=int, default=None, metavar="N", help="the largest code of a 16-bit data set (default 65535)")
    add_arguments(ap)
    ap.add_argument("--stats", action="store_true", help="print valid=, flying=, speckle= and regions= per file")
    a = ap.parse_args(argv)
    if a.depth_max is not None and a.depth_bits != 16:
        ap.error("--depth-max needs --depth-bits 16")
    if a.depth_max is not None and not 1 <= a.depth_max <= 65535:
        ap.error(f"--depth-max {a.depth_max} must be in [1, 65535]")
    if os.path.abspath(a.out) == os.path.abspath(a.depth):
        ap.error("--out is --depth: the cleaned maps would overwrite the sensor's")
    cleaner = cleaner_of(a, ap)
    top = 255 if a.depth_bits == 8 else 65535 if a.depth_max is None else a.depth_max
    if cleaner.tolerance > top:
        ap.error(f"--tolerance {cleaner.tolerance} is above the largest code {top}")
    return a, ap, cleaner


def stats_line(counts) -> str:
    """valid= flying= speckle= regions= of one image's four counts (an int32 row read as unsigned)"""
    return " ".join(f"{k}={int(v)}" for k, v in zip(STATS, np.asarray(counts).view(np.uint32)))


def main(argv=None, emit=print):
    a, ap, cleaner = parse_args(argv)
    if not os.path.isdir(a.depth):
        ap.error(f"--depth {a.depth} is not a directory")
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: codon_amd has no CPU fallback")
    depth_max = 65535 if a.depth_max is None else a.depth_max
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    for name in sorted(os.listdir(a.depth)):
        plane = io.read_depth_plane(os.path.join(a.depth, name), a.depth_bits, depth_max)
        codes = torch.from_numpy((plane.view(np.int16) if plane.dtype == np.uint16 else plane).copy()).to(dev)
        got = cleaner(codes, depth_max if a.depth_bits == 16 else None, stats=a.stats)
        out, counts = got if a.stats else (got, None)
        if a.depth_bits == 16:
            io.write_depth16(os.path.join(a.out, name), out.cpu().numpy().view(np.uint16))
        else:
            io.write_gray(os.path.join(a.out, name), out.cpu().numpy())
        emit(f"{name} {stats_line(counts.cpu().numpy()[0])}" if a.stats else name)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
