"""Temporal filtering of a FIXED camera's depth sequence: the step in front of `python -m codon_amd.clean`, in the
sensor's own frame.  Range noise on a static pixel averages out over frames; a pixel that is valid in one frame and a hole in the
next (flicker) takes the value that stood in the frames around it; a one-frame spike is rejected by the frames around it, whatever
its spatial support.  The recommended order is temporal -> clean -> smooth -> register.

    python -m codon_amd.temporal --depth DIR --out DIR [--depth-bits {8,16}] [--depth-max N] [--window W] [--causal]
                                 [--tolerance CODES] [--tolerance-rel F] [--min-count M] [--min-fill F] [--block FRAMES] [--stream]
                                 [--stats]

The files of --depth in the order of their names are ONE sequence from one camera that stands still.  The definition, in integers
(tests/temporal_ref.py; csrc/temporal.hip): the window of frame t is the --window frames centred on it (--causal: t and the
W - 1 before it), cut at the sequence's ends.  Two samples are linked under clean's rule: both valid, codes at most tolerance +
tolerance_rel * the smaller code apart.  A valid sample with at least --min-count window samples linked to it (itself among them;
the count is capped by the window's frames) becomes their mean, rounded half up; with fewer it is REJECTED (1: off).  A hole or a
rejected sample becomes the rounded mean of the samples linked to the lower median of the window's valid samples, if there are at
least --min-fill valid samples and at least that many linked to the median, else 0 (0: filling off; not capped at the ends).  Every
read is of the input: one pass, not idempotent.  An output of the first kind differs from its input by at most the tolerance, so
a moving occlusion edge never yields a code between the two surfaces.  The four defaults of the tolerances, --min-count and
--min-fill are untuned.  A live stream, or a recording too long to hold, goes through frame by frame: TemporalStream (DESIGN
12.24) keeps the window on the device, --stream runs the files through it one at a time, and `python -m codon_amd.register
--temporal` chains it with clean and register on one upload per file.  Not handled: a moving camera; more than one sequence per
call or per stream object; checkpointing a stream's ring to disk; confidence images; windows beyond 15; motion compensation; a
queue of colour images to pair with outputs that lag by `ahead` frames (the caller holds its own)."""
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

MAX_WINDOW, MAX_FRAMES, MAX_SIDE = 15, 4096, 4096
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


MAX_STREAM_FRAMES = (1 << 31) - 1


class TemporalStream:
    """A TemporalFilter over a live stream, one frame per call, the window resident on the device: 16 planes and
    two counter words, whatever the length.  Frame t is final once frame t + filt.ahead is in, so push() answers `latency` =
    filt.ahead frames late and flush() hands out the rest; the outputs and statistics are those of filt(whole sequence), bit for
    bit (tests/temporal_ref.py), for any number of frames.

        s = TemporalStream(filt, (h, w), torch.int16, depth_max=10000)
        for frame in camera:                # (h, w) codes of the stream's dtype on the stream's device
            o = s.push(frame)               # None for the first `ahead` frames, then frame (s.frames - 1 - ahead)
        rest = s.flush()                    # the last min(ahead, frames) outputs, in order; the stream is then closed
        s.reset()                           # open again, at frame 0

    dtype: torch.uint8, int16 or uint16 (u16 codes); device: a HIP device with its index (default cuda:0).  frames, emitted:
    host mirrors of what went in and came out.  One object is ONE sequence at a time; a colour image that belongs to an output
    is the caller's to hold for `latency` frames.  The device memory is allocated by the first push."""

    def __init__(self, filt: TemporalFilter, shape, dtype, depth_max: int = None, device=None):
        who = self.who = "temporal_push"
        if not isinstance(filt, TemporalFilter):
            raise ValueError(f"{who}: filt {filt!r} (a TemporalFilter)")
        try:
            h, w = shape
        except (TypeError, ValueError):
            raise ValueError(f"{who}: shape {shape!r} ((h, w), 1..{MAX_SIDE} each way)") from None
        what = f"(h, w), 1..{MAX_SIDE} each way"
        self.shape = (integer(who, "shape", h, 1, MAX_SIDE, what), integer(who, "shape", w, 1, MAX_SIDE, what))
        if dtype not in (torch.uint8, torch.int16, torch.uint16):
            raise ValueError(f"{who}: dtype {dtype!r} (torch.uint8, or torch.int16 / torch.uint16 for u16 codes)")
        if dtype == torch.uint8 and depth_max not in (None, 255):
            raise ValueError(f"{who}: depth_max {depth_max!r} with 8-bit codes")
        self.top = 255 if dtype == torch.uint8 else 65535 if depth_max is None else depth_max
        io.check_depth_max(self.top)
        if filt.tolerance > self.top:
            raise ValueError(f"{who}: tolerance {filt.tolerance} above the largest code {self.top}")
        self.filt, self.dtype, self.depth_max = filt, dtype, depth_max
        self.fmt = L.FILL_U8 if dtype == torch.uint8 else L.FILL_U16
        self.device = torch.device("cuda:0" if device is None else device)
        if self.device.type != "cuda" or self.device.index is None:
            raise ValueError(f"{who}: device {device!r} (a HIP device with its index, such as 'cuda:0')")
        self.latency = filt.ahead
        self.frames = self.emitted = 0
        self.closed = False
        self._ring = self._state = self._spare = None

    def _plane(self, who, name, t):
        """t is a plane of the stream's shape, dtype and device; refusals by name, in that order"""
        h, w = self.shape
        if tuple(t.shape) != (h, w):
            raise ValueError(f"{who}: {name} of shape {tuple(t.shape)}, the stream's is ({h}, {w})")
        if t.dtype != self.dtype:
            raise ValueError(f"{who}: {name} of {t.dtype}, the stream's is {self.dtype}")

    def _step(self, src, stats, out):
        """One step of the library (src None: a flush step) -> (out, counts or None)"""
        who, f, dev = self.who, self.filt, self.device
        h, w = self.shape
        with ops._on(dev):
            if self._ring is None:
                if torch.cuda.is_current_stream_capturing():
                    raise RuntimeError(f"{who}: the first push allocates the ring: push one frame before a capture")
                self._ring = torch.empty((L.load().codon_temporal_ring_frames(), h, w), dtype=self.dtype, device=dev)
                self._state = torch.zeros(2, dtype=torch.int32, device=dev)
            if out is None:
                out = torch.empty((h, w), dtype=self.dtype, device=dev)
            counts = torch.empty(4, dtype=torch.int32, device=dev) if stats else None
            P_ = C.c_void_p
            L.check(L.load().codon_temporal_push(h, w, None if src is None else P_(src.data_ptr()), self.fmt, self.top, f.back, f.ahead,
                                                 f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill,
                                                 P_(self._ring.data_ptr()), P_(self._state.data_ptr()), P_(out.data_ptr()),
                                                 P_(counts.data_ptr()) if stats else None, ops._stream(dev)), who)
        return out, counts

    def push(self, codes: torch.Tensor, stats: bool = False, out: torch.Tensor = None):
        """codes: (h, w) codes of the stream's dtype on the stream's device, the next frame; it is not modified -> None while
        fewer than ahead + 1 frames are in, then frame (frames - 1 - ahead): (h, w) codes, or with stats=True (codes, int32 (4,)
        on the device: valid inputs, rejected, filled, changed).  out: a plane to write into instead of a new one (left as it
        was while the answer is None).  Two launches, no workspace, no host synchronisation.
        Under a graph capture `out` is required and is returned whatever the frame index, which lives on the device: one
        captured push replays for every later frame; tell the mirrors with replayed()."""
        who = self.who
        if self.closed:
            raise RuntimeError(f"{who}: a push after flush(): the stream is closed (reset() opens it at frame 0)")
        if self.frames >= MAX_STREAM_FRAMES:
            raise RuntimeError(f"{who}: {self.frames} frames are in (at most 2^31 - 1: reset())")
        p = K.code_planes(who, codes, self.depth_max, "(h,w) uint8 codes, or u16 codes as int16 / uint16")
        self._plane(who, "a frame", codes)
        capturing = torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()
        if out is not None:
            self._plane(who, "out", out)
            if not out.is_contiguous():
                raise ValueError(f"{who}: out is not contiguous")
        elif capturing:
            raise RuntimeError(f"{who}: under a graph capture push needs out=")
        for name, t in (("a frame", codes), ("out", out)):
            if t is not None and t.device != self.device:
                raise RuntimeError(f"{who}: {name} on {t.device}, the stream on {self.device}")
        final = self.frames >= self.latency                    # this push makes a frame final
        got, counts = self._step(p.src, stats, out if (final or capturing) else self._spare_plane())
        self.frames += 1
        if not (final or capturing):
            return None
        self.emitted += final
        return (got, counts) if stats else got

    def _spare_plane(self):
        """The plane a step that emits nothing is given: a caller's `out` stays out of the call"""
        if self._spare is None:
            self._spare = torch.empty(self.shape, dtype=self.dtype, device=self.device)
        return self._spare

    def flush(self, stats: bool = False):
        """The outputs still owed, frames emitted .. frames - 1 in order: a list of min(ahead, frames) planes, or of (codes,
        counts) with stats=True; the stream is then closed.  Two launches per output."""
        rest = []
        while self.emitted < self.frames:
            got, counts = self._step(None, stats, None)
            self.emitted += 1
            rest.append((got, counts) if stats else got)
        self.closed = True
        return rest

    def reset(self):
        """The counters to 0 (on the current stream of the device); the stream is open again"""
        if self._state is not None:
            with ops._on(self.device):
                self._state.zero_()
        self.frames = self.emitted = 0
        self.closed = False

    def replayed(self, n: int = 1):
        """n replays of a captured push have run: the host mirrors follow"""
        n = integer(self.who, "n", n, 0, MAX_STREAM_FRAMES - self.frames, "replays, at least 0; at most 2^31 - 1 frames in all")
        self.frames += n
        self.emitted = max(0, self.frames - self.latency)

    def sync_frames(self) -> int:
        """The device's own count of the frames pushed, read back -- a HOST SYNCHRONISATION -- into the mirrors"""
        if self._state is not None:
            pushed, flushed = (int(v) for v in self._state.cpu().numpy().view(np.uint32))
            self.frames = pushed
            self.emitted = min(pushed, max(0, pushed - self.latency) + flushed)
        return self.frames

    def filter(self, frames, stats: bool = False):
        """Push every frame of an iterable, then flush: yields one output per input, in order"""
        for frame in frames:
            got = self.push(frame, stats=stats)
            if got is not None:
                yield got
        yield from self.flush(stats=stats)


# ---- the command line ---------------------------------------------------------------------------------------------------------------

def add_arguments(ap, prefix: str = ""):
    """--window, --causal, --tolerance, --tolerance-rel, --min-count, --min-fill under `prefix` ("temporal-" for register's)"""
    ap.add_argument(f"--{prefix}window", type=int, default=DEFAULTS["window"], metavar="W",
                    help=f"frames in the window, 1..{MAX_WINDOW}: odd and centred on the frame, or with --{prefix}causal any (default 5)")
    ap.add_argument(f"--{prefix}causal", action="store_true", help="the window is the frame and the W - 1 before it")
    ap.add_argument(f"--{prefix}tolerance", type=int, default=DEFAULTS["tolerance"], metavar="CODES",
                    help="two samples are linked when their codes differ by at most this ... (default 2, untuned)")
    ap.add_argument(f"--{prefix}tolerance-rel", type=float, default=DEFAULTS["tolerance_rel"], metavar="F",
                    help="... plus this fraction of the smaller code (default 0.02, untuned)")
    ap.add_argument(f"--{prefix}min-count", type=int, default=DEFAULTS["min_count"], metavar="M",
                    help="a sample with fewer linked samples in its window, itself among them, is rejected; 1: off (default 2, untuned)")
    ap.add_argument(f"--{prefix}min-fill", type=int, default=DEFAULTS["min_fill"], metavar="F",
                    help="a hole is filled from at least this many valid samples linked to the window's median; 0: off (default 2, untuned)")


def filter_of(a, ap, prefix: str = "") -> TemporalFilter:
    """The TemporalFilter of parsed arguments; what it refuses is the parser's error"""
    get = lambda n: getattr(a, (prefix + n).replace("-", "_"))            # noqa: E731
    try:
        return TemporalFilter(get("window"), get("causal"), get("tolerance"), get("tolerance-rel"), get("min-count"), get("min-fill"))
    except ValueError as e:
        ap.error(str(e).replace("TemporalFilter: ", "--" + prefix).replace("_", "-"))


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m codon_amd.temporal", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--depth", required=True, metavar="DIR", help="one fixed camera's depth maps, in the order of their names")
    ap.add_argument("--out", required=True, metavar="DIR", help="where the filtered maps go, under the same file names")
    K.add_depth_args(ap)
    add_arguments(ap)
    ap.add_argument("--block", type=int, default=BLOCK, metavar="FRAMES",
                    help=f"frames filtered per upload, which bounds the device memory; the output does not depend on it (default {BLOCK}); "
                    "not looked at with --stream")
    ap.add_argument("--stream", action="store_true",
                    help="read, filter and write one file at a time (TemporalStream): 16 planes of device memory whatever the length, "
                    "the same files and lines")
    ap.add_argument("--stats", action="store_true", help="print valid=, rejected=, filled= and changed= per file")
    a = ap.parse_args(argv)
    a.top = K.depth_args_of(ap, a)
    if os.path.abspath(a.out) == os.path.abspath(a.depth):
        ap.error("--out is --depth: the filtered maps would overwrite the sensor's")
    filt = filter_of(a, ap)
    if filt.tolerance > a.top:
        ap.error(f"--tolerance {filt.tolerance} is above the largest code {a.top}")
    if not a.stream and not 1 <= a.block <= MAX_FRAMES - (MAX_WINDOW - 1):
        ap.error(f"--block {a.block} must be in [1, {MAX_FRAMES - (MAX_WINDOW - 1)}]")
    return a, ap, filt


def stats_line(counts) -> str:
    """valid= rejected= filled= changed= of one frame's four counts (an int32 row read as unsigned)"""
    return " ".join(f"{k}={int(v)}" for k, v in zip(STATS, np.asarray(counts).view(np.uint32)))


def blocks(n: int, block: int, back: int, ahead: int):
    """(first, stop, lo, hi) of every block of a sequence of n frames: frames [first, stop) are written from an upload of frames
    [lo, hi), the block with `back` frames before it and `ahead` after -- every window of the block, whole"""
    return [(a, min(a + block, n), max(0, a - back), min(n, min(a + block, n) + ahead)) for a in range(0, n, block)]


def one_shape(ap, names, i, shape, first):
    """File i of a sequence has the first file's shape, or the parser's error"""
    if tuple(shape) != tuple(first):
        ap.error(f"{names[i]} is {shape[0]}x{shape[1]}, {names[0]} is {first[0]}x{first[1]}: "
                 "one sequence from one camera has one shape")


def stream_files(filt, ap, directory, depth_bits, top, depth_max, dev, stats=False):
    """(name, filtered codes on dev, counts or None) for every depth map of a directory, the files in the order of their names
    being one sequence: each is read, uploaded and pushed once, and a frame comes out `filt.ahead` files late, under its own name"""
    names = sorted(os.listdir(directory))
    s = None
    for i, name in enumerate(names):
        plane = io.read_depth_plane(os.path.join(directory, name), depth_bits, top)
        if s is None:
            s = TemporalStream(filt, plane.shape, torch.uint8 if plane.dtype == np.uint8 else torch.int16, depth_max, dev)
        one_shape(ap, names, i, plane.shape, s.shape)
        got = s.push(K.codes_tensor(plane).to(dev), stats=stats)
        if got is not None:
            yield (names[i - s.latency], *(got if stats else (got, None)))
    if s is not None:
        first = s.emitted
        for j, got in enumerate(s.flush(stats=stats)):
            yield (names[first + j], *(got if stats else (got, None)))


def main(argv=None, emit=print):
    a, ap, filt = parse_args(argv)
    K.require_dir(ap, "depth", a.depth)
    names = sorted(os.listdir(a.depth))
    dev = K.require_gpu()
    os.makedirs(a.out, exist_ok=True)
    if a.stream:
        for name, out, counts in stream_files(filt, ap, a.depth, a.depth_bits, a.top, a.depth_max, dev, a.stats):
            K.write_codes(os.path.join(a.out, name), out)
            emit(f"{name} {stats_line(counts.cpu().numpy())}" if a.stats else name)
        return 0
    held: dict = {}                                 # frame index -> host plane, the frames two neighbouring blocks share among them
    shape = None
    for first, stop, lo, hi in blocks(len(names), a.block, filt.back, filt.ahead):
        held = {i: held[i] for i in range(lo, hi) if i in held}
        for i in range(lo, hi):
            if i not in held:
                held[i] = io.read_depth_plane(os.path.join(a.depth, names[i]), a.depth_bits, a.top)
                shape = held[i].shape if shape is None else shape
                one_shape(ap, names, i, held[i].shape, shape)
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
