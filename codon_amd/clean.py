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
read.  A fixed camera's sequence is filtered over time by the step in front of this one, `python -m codon_amd.temporal` (DESIGN
12.23), and what survives is smoothed in space by the step behind it, `python -m codon_amd.smooth`: the recommended
order is temporal -> clean -> smooth -> register."""
from __future__ import annotations

import argparse
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import codes as K
from . import ops
from .codes import integer, rel_q16

MAX_SUPPORT, MAX_REGION, MAX_REL_Q16 = 8, 1 << 24, 65535
STATS = ("valid", "flying", "speckle", "regions")
DEFAULTS = dict(tolerance=2, tolerance_rel=0.02, min_support=3, min_region=16)


class Cleaner:
    """clean(codes) removes flying pixels and speckles from a batch of the depth camera's own planes.  tolerance: codes;
    tolerance_rel: a fraction of the smaller code; min_support: K of rule 1 (0: off); min_region: N of rule 2 (0, 1: off)."""

    def __init__(self, tolerance: int = 2, tolerance_rel: float = 0.02, min_support: int = 3, min_region: int = 16):
        who = "Cleaner"
        self.tolerance = integer(who, "tolerance", tolerance, 0, 65535, "an integer number of codes, 0 .. the largest code")
        self.tolerance_rel = tolerance_rel
        self.tolerance_rel_q16 = rel_q16(who, tolerance_rel)
        self.min_support = integer(who, "min_support", min_support, 0, MAX_SUPPORT, f"an integer in 0..{MAX_SUPPORT}")
        self.min_region = integer(who, "min_region", min_region, 0, MAX_REGION, f"an integer in 0..{MAX_REGION}")

    def __call__(self, codes: torch.Tensor, depth_max: int = None, stats: bool = False):
        """codes: (h, w) or (B, h, w) uint8 codes, or u16 codes as int16 / uint16 (read as unsigned), 0 a hole, on a GPU -> codes
        of the argument's shape and dtype, each the argument's code or 0; the argument is not modified.  stats=True: (codes,
        int32 (B, 4) on the device: valid inputs, pixels removed by rule 1, pixels removed by rule 2, components removed by
        rule 2).  Two launches with rule 2 off, four with it on; no host synchronisation."""
        who = "clean_depth"
        p = K.code_planes(who, codes, depth_max)
        if self.tolerance > p.top:
            raise ValueError(f"{who}: tolerance {self.tolerance} above the largest code {p.top}")
        dev, out = p.dev, p.out()
        counts = torch.empty((p.B, 4), dtype=torch.int32, device=dev) if stats else None
        P_ = C.c_void_p
        with ops._on(dev):
            ws = K.workspace(who, "codon_clean_workspace_bytes", dev, p.B, p.h, p.w, batched=True)
            L.check(L.load().codon_clean_depth(p.B, p.h, p.w, p.ptr, p.fmt, p.top, self.tolerance,
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
    K.add_depth_args(ap)
    add_arguments(ap)
    ap.add_argument("--stats", action="store_true", help="print valid=, flying=, speckle= and regions= per file")
    a = ap.parse_args(argv)
    a.top = K.depth_args_of(ap, a)
    if os.path.abspath(a.out) == os.path.abspath(a.depth):
        ap.error("--out is --depth: the cleaned maps would overwrite the sensor's")
    cleaner = cleaner_of(a, ap)
    if cleaner.tolerance > a.top:
        ap.error(f"--tolerance {cleaner.tolerance} is above the largest code {a.top}")
    return a, ap, cleaner


def stats_line(counts) -> str:
    """valid= flying= speckle= regions= of one image's four counts (an int32 row read as unsigned)"""
    return " ".join(f"{k}={int(v)}" for k, v in zip(STATS, np.asarray(counts).view(np.uint32)))


def main(argv=None, emit=print):
    a, ap, cleaner = parse_args(argv)
    K.require_dir(ap, "depth", a.depth)
    dev = K.require_gpu()
    os.makedirs(a.out, exist_ok=True)
    for name, codes in K.depth_files(a.depth, a.depth_bits, a.top, dev):
        got = cleaner(codes, a.depth_max, stats=a.stats)
        out, counts = got if a.stats else (got, None)
        K.write_codes(os.path.join(a.out, name), out)
        emit(f"{name} {stats_line(counts.cpu().numpy()[0])}" if a.stats else name)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
