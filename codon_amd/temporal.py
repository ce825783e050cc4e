"""Temporal filtering of a FIXED camera's depth sequence: the step in front of `python -m codon_amd.clean`, in the
sensor's own frame.  Range noise on a static pixel averages out over frames; a pixel that is valid in one frame and a hole in the
next (flicker) takes the value that stood in the frames around it; a one-frame spike is rejected by the frames around it, whatever
its spatial support.  The recommended order is temporal -> clean -> register.

    python -m codon_amd.temporal --depth DIR --out DIR [--depth-bits {8,16}] [--depth-max N] [--window W] [--causal]
                                 [--tolerance CODES] [--tolerance-rel F] [--min-count M] [--min-fill F] [--block FRAMES] [--stats]

The files of --depth in the order of their names are ONE sequence from one camera that stands still.  The definition, in integers
(tests/temporal_ref.py; csrc/temporal.hip): the window of frame t is the --window frames centred on it (--causal: t and the
W - 1 before it), cut at the sequence's ends.  Two samples are linked under clean's rule: both valid, codes at most tolerance +
tolerance_rel * the smaller code apart.  A valid sample with at least --min-count window samples linked to it (itself among them;
the count is capped by the window's frames) becomes their mean, rounded half up; with fewer it is REJECTED (1: off).  A hole or a
rejected sample becomes the rounded mean of the samples linked to the lower median of the window's valid samples, if there are at
least --min-fill valid samples and at least that many linked to the median, else 0 (0: filling off; not capped at the ends).  Every
read is of the input: one pass, not idempotent.  An output of the first kind differs from its input by at most the tolerance, so
a moving occlusion edge never yields a code between the two surfaces.  The four defaults of the tolerances, --min-count and
--min-fill are untuned.  Not handled: a moving camera; more than one sequence per call; a stateful live push(frame) interface;
confidence images; windows beyond 15; motion compensation."""
from __future__ import annotations

import argparse
import ctypes as C
import os

import numpy as np
import torch

from . import _lib as L
from . import codes as K
from . import io, ops
from .codes import integer, rel_q16

MAX_WINDOW, MAX_FRAMES = 15, 4096
STATS = ("valid", "rejected", "filled", "changed")
DEFAULTS = dict(window=5, causal=False, tolerance=2, tolerance_rel=0.02, min_count=2, min_fill=2)
BLOCK = 256


class TemporalFilter:
    """filter(codes) filters a (T, h, w) sequence of a fixed camera's planes over time.  window: frames, odd and centred, or with
    causal=True any number, the frame and those before it; back=, ahead=: the window's two sides spelled out instead.  tolerance:
    codes; tolerance_rel: a fraction of the smaller code; min_count: M of rejection (1: off); min_fill: F of filling (0: off).  The
    last four defaults are untuned."""

    def __init__(self, window: int = 5, causal: bool = False, tolerance: int = 2, tolerance_rel: float = 0.02, min_count: int = 2,
                 min_fill: int = 2, back: int = None, ahead: int = None):
        who = "TemporalFilter"
        if back is not None or ahead is not None:
            sides = f"integers of at least 0 that sum to at most {MAX_WINDOW - 1}, given together"
            self.back = integer(who, "back", back, 0, MAX_WINDOW - 1, sides)
            self.ahead = integer(who, "ahead", ahead, 0, MAX_WINDOW - 1 - self.back, sides)
        else:
            if not isinstance(causal, (bool, np.bool_)):
                raise ValueError(f"{who}: causal {causal!r} (True or False)")
            w = integer(who, "window", window, 1, MAX_WINDOW, f"an integer in 1..{MAX_WINDOW}, odd unless causal")
            if not causal and w % 2 == 0:
                raise ValueError(f"{who}: window {window!r} (an integer in 1..{MAX_WINDOW}, odd unless causal)")
            self.back, self.ahead = (w - 1, 0) if causal else (w // 2, w // 2)
        self.window = self.back + self.ahead + 1
        self.tolerance = integer(who, "tolerance", tolerance, 0, 65535, "an integer number of codes, 0 .. the largest code")
        self.tolerance_rel = tolerance_rel
        self.tolerance_rel_q16 = rel_q16(who, tolerance_rel)
        self.min_count = integer(who, "min_count", min_count, 1, MAX_WINDOW, f"an integer in 1..{MAX_WINDOW}")
        self.min_fill = integer(who, "min_fill", min_fill, 0, MAX_WINDOW, f"an integer in 0..{MAX_WINDOW}")

    def __call__(self, codes: torch.Tensor, depth_max: int = None, stats: bool = False):
        """codes: (T, h, w) uint8 codes, or u16 codes as int16 / uint16 (read as unsigned), 0 a hole, frame order being time, on a
        GPU; (h, w) is a sequence of one frame -> codes of the argument's shape and dtype; the argument is not modified.
        stats=True: (codes, int32 (T, 4) on the device: valid inputs, rejected, filled, changed).  Two launches, no workspace,
        no host synchronisation."""
        who = "temporal_depth"
        p = K.code_planes(who, codes, depth_max)
        if p.B > MAX_FRAMES:
            raise ValueError(f"{who}: a sequence of {p.B} frames (1..{MAX_FRAMES})")
        if p.B * p.h * p.w >= 1 << 31:
            raise ValueError(f"{who}: a sequence of {p.B * p.h * p.w} codes ({p.B} frames of {p.h}x{p.w}; below 2^31)")
        if self.tolerance > p.top:
            raise ValueError(f"{who}: tolerance {self.tolerance} above the largest code {p.top}")
        dev, out = p.dev, p.out()
        counts = torch.empty((p.B, 4), dtype=torch.int32, device=dev) if stats else None
        P_ = C.c_void_p
        with ops._on(dev):
            L.check(L.load().codon_temporal_depth(p.B, p.h, p.w, p.ptr, p.fmt, p.top, self.back, self.ahead, self.tolerance,
                                                  self.tolerance_rel_q16, self.min_count, self.min_fill, P_(out.data_ptr()),
                                                  P_(counts.data_ptr()) if stats else None, ops._stream(dev)), who)
        return (out, counts) if stats else out


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m codon_amd.temporal", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", required=True, metavar="DIR", help="one fixed camera's depth maps, in the order of their names")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the filtered maps go, under the same file names")
    K.add_depth_args(ap)
    ap.add_argument("--window", type=int, default=DEFAULTS["window"], metavar="W",
                    help=f"frames in the window, 1..{MAX_WINDOW}: odd and centred on the frame, or with --causal any (default 5)")
    ap.add_argument("--causal", action="store_true", help="the window is the frame and the W - 1 before it")
    ap.add_argument("--tolerance", type=int, default=DEFAULTS["tolerance"], metavar="CODES",
                    help="two samples are linked when their codes differ by at most this ... (default 2, untuned)")
    ap.add_argument("--tolerance-rel", type=float, default=DEFAULTS["tolerance_rel"], metavar="F",
                    help="... plus this fraction of the smaller code (default 0.02, untuned)")
    ap.add_argument("--min-count", type=int, default=DEFAULTS["min_count"], metavar="M",
                    help="a sample with fewer linked samples in its window, itself among them, is rejected; 1: off (default 2, untuned)")
    ap.add_argument("--min-fill", type=int, default=DEFAULTS["min_fill"], metavar="F",
                    help="a hole is filled from at least this many valid samples linked to the window's median; 0: off (default 2, untuned)")
    ap.add_argument("--block", type=int, default=BLOCK, metavar="FRAMES",
                    help=f"frames filtered per upload, which bounds the device memory; the output does not depend on it (default {BLOCK})")
    ap.add_argument("--stats", action="store_true", help="print valid=, rejected=, filled= and changed= per file")
    a = ap.parse_args(argv)
    a.top = K.depth_args_of(ap, a)
    if os.path.abspath(a.out) == os.path.abspath(a.depth):
        ap.error("--out is --depth: the filtered maps would overwrite the sensor's")
    try:
        filt = TemporalFilter(a.window, a.causal, a.tolerance, a.tolerance_rel, a.min_count, a.min_fill)
    except ValueError as e:
        ap.error(str(e).replace("TemporalFilter: ", "--").replace("_", "-"))
    if filt.tolerance > a.top:
        ap.error(f"--tolerance {filt.tolerance} is above the largest code {a.top}")
    if not 1 <= a.block <= MAX_FRAMES - (MAX_WINDOW - 1):
        ap.error(f"--block {a.block} must be in [1, {MAX_FRAMES - (MAX_WINDOW - 1)}]")
    return a, ap, filt


def stats_line(counts) -> str:
    """valid= rejected= filled= changed= of one frame's four counts (an int32 row read as unsigned)"""
    return " ".join(f"{k}={int(v)}" for k, v in zip(STATS, np.asarray(counts).view(np.uint32)))


def blocks(n: int, block: int, back: int, ahead: int):
    """(first, stop, lo, hi) of every block of a sequence of n frames: frames [first, stop) are written from an upload of frames
    [lo, hi), the block with `back` frames before it and `ahead` after -- every window of the block, whole"""
    return [(a, min(a + block, n), max(0, a - back), min(n, min(a + block, n) + ahead)) for a in range(0, n, block)]


def main(argv=None, emit=print):
    a, ap, filt = parse_args(argv)
    K.require_dir(ap, "depth", a.depth)
    names = sorted(os.listdir(a.depth))
    dev = K.require_gpu()
    os.makedirs(a.out, exist_ok=True)
    held: dict = {}                                 # frame index -> host plane, the frames two neighbouring blocks share among them
    shape = None
    for first, stop, lo, hi in blocks(len(names), a.block, filt.back, filt.ahead):
        held = {i: held[i] for i in range(lo, hi) if i in held}
        for i in range(lo, hi):
            if i not in held:
                held[i] = io.read_depth_plane(os.path.join(a.depth, names[i]), a.depth_bits, a.top)
                shape = held[i].shape if shape is None else shape
                if held[i].shape != shape:
                    ap.error(f"{names[i]} is {held[i].shape[0]}x{held[i].shape[1]}, {names[0]} is {shape[0]}x{shape[1]}: "
                             "one sequence from one camera has one shape")
        seq = K.codes_tensor(np.stack([held[i] for i in range(lo, hi)])).to(dev)
        got = filt(seq, a.depth_max, stats=a.stats)
        out, counts = got if a.stats else (got, None)
        rows = counts.cpu().numpy() if a.stats else None
        for i in range(first, stop):
            K.write_codes(os.path.join(a.out, names[i]), out[i - lo])
            emit(f"{names[i]} {stats_line(rows[i - lo])}" if a.stats else names[i])
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
