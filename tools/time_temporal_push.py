"""What one push of the temporal stream costs, on the GPU: codon_amd.temporal.TemporalStream.push, eager and as a
graph replay, beside two yardsticks taken in the SAME process -- a `copy_` of one plane (every code of a frame read once and
written once) and the sequence kernel's time per frame on 64 frames of the same pattern (TemporalFilter's call over 64).  Legs
alternate after a warm-up leg, and the spread of every leg is printed beside the medians: median [min ... max] of 20 windows of
20 calls, device events around back-to-back calls enqueued from Python.

    python tools/time_temporal_push.py [--json FILE]    424 x 512 u16 and 480 x 640 u8; windows (2, 2), (4, 0) and (14, 0); the
                                                        `calm` and `flicker` patterns of tools/time_temporal.py

A push cycles through the 64 frames of the pattern with a caller's out=; the graph leg replays one captured push per frame of the
cycle (64 graphs of two kernel nodes each, captured once), so that eager and replayed pushes filter the same contents.  The stream
is past its first `ahead` frames when the clock starts: every timed push emits a frame.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.temporal import TemporalFilter, TemporalStream  # noqa: E402
from time_fill import spread  # noqa: E402
from time_temporal import PATTERNS, SEQUENCES, sequence  # noqa: E402

SIDES = ((2, 2), (4, 0), (14, 0))                                   # (back, ahead)
WARMUP, WINDOWS, CALLS = 10, 20, 20


def variants(T, h, w, bits, pattern, back, ahead, dev):
    codes = torch.from_numpy(sequence(np.random.default_rng(T + h), T, h, w, bits, pattern)).to(dev)
    filt = TemporalFilter(back=back, ahead=ahead)
    sink, out = torch.empty_like(codes[0]), torch.empty_like(codes[0])
    eager, replayed = TemporalStream(filt, (h, w), codes.dtype), TemporalStream(filt, (h, w), codes.dtype)
    for s in (eager, replayed):
        for t in range(T):                                           # past the first frames, the ring full
            s.push(codes[t], out=out)
    torch.cuda.synchronize(dev)
    graphs, pool = [], None
    for t in range(T):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, pool=pool):
            replayed.push(codes[t], out=out)
        pool = g.pool()
        graphs.append(g)
    turn = {"eager": 0, "graph": 0}

    def push():
        eager.push(codes[turn["eager"] % T], out=out)
        turn["eager"] += 1

    def replay():
        graphs[turn["graph"] % T].replay()
        turn["graph"] += 1

    return {"copy_ of a plane": lambda: sink.copy_(codes[0]), "push": push, "push, graph replay": replay,
            "sequence call / 64": lambda: filt(codes)}, T


def time_pushes():
    dev = torch.device("cuda:0")
    rows = []
    for T, h, w, bits in SEQUENCES:
        for pattern in PATTERNS:
            for back, ahead in SIDES:
                legs, frames = variants(T, h, w, bits, pattern, back, ahead, dev)
                name = f"{h}x{w} u{bits} {pattern} window ({back}, {ahead})"
                for fn in legs.values():
                    for _ in range(WARMUP):
                        fn()
                torch.cuda.synchronize(dev)
                times = {k: [] for k in legs}
                for _ in range(WINDOWS):
                    for k, fn in legs.items():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        for _ in range(CALLS):
                            fn()
                        e1.record()
                        e1.synchronize()
                        per = frames if k.startswith("sequence") else 1
                        times[k].append(e0.elapsed_time(e1) * 1e3 / CALLS / per)
                for k, v in times.items():
                    rows.append({"plane": f"{h}x{w}", "bits": bits, "pattern": pattern, "back": back, "ahead": ahead, "leg": k, "us": v})
                    print(f"{name} {k}: {spread(v)} us per frame", flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    rows = time_pushes()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
