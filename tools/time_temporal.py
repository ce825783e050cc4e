"""What the temporal filter of a depth sequence costs, on the GPU: codon_amd.temporal.TemporalFilter's call beside a
`copy_` of the same input bytes to a tensor of the output's size in ONE process, so that the copy -- every code read once and
written once, the floor of the filter's bytes -- is the yardstick of that box.  Legs alternate after a warm-up leg, and the spread
of every leg is printed beside the medians.

    python tools/time_temporal.py calls [--json FILE]   time per call for a 64 x 424 x 512 u16 and a 64 x 480 x 640 u8 sequence, at
                                                        windows 5 and 15, a noisy static scene with 5 % flicker holes and spikes
                                                        and the same without holes or spikes (no pixel takes the median's
                                                        branch), with statistics at window 5: device events around windows of
                                                        back-to-back calls, enqueued from Python; the ratio to the copy beside it
    python tools/time_temporal.py kernels               a few hundred calls of the same and nothing else: the run to trace
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
from codon_amd.temporal import TemporalFilter  # noqa: E402
from time_fill import spread  # noqa: E402

SEQUENCES = ((64, 424, 512, 16), (64, 480, 640, 8))                 # T, h, w, code bits
PATTERNS = ("flicker", "calm")
WARMUP, WINDOWS, CALLS = 10, 20, 20


def sequence(g, T, h, w, bits, pattern):
    """T frames of a static scene: a smooth surface under +- 3 codes (u16, millimetres) or +- 1 (u8) of fresh noise per frame;
    `flicker`: 5 % holes and 0.5 % samples of a random code per frame"""
    yy, xx = np.mgrid[0:h, 0:w]
    if bits == 16:
        c = np.rint(2750 + 1250 * np.sin(0.011 * yy) * np.cos(0.007 * xx)).astype(np.int64)[None] + g.integers(-3, 4, size=(T, h, w))
    else:
        c = np.rint(128 + 100 * np.sin(0.011 * yy) * np.cos(0.007 * xx)).astype(np.int64)[None] + g.integers(-1, 2, size=(T, h, w))
    if pattern == "flicker":
        spikes = g.uniform(size=(T, h, w)) < 0.005
        c[spikes] = g.integers(1, 256 if bits == 8 else 10000, size=int(spikes.sum()))
        c[g.uniform(size=(T, h, w)) < 0.05] = 0
    return c.astype(np.uint8) if bits == 8 else c.astype(np.uint16).view(np.int16)


def call_variants(T, h, w, bits, pattern, dev):
    codes = torch.from_numpy(sequence(np.random.default_rng(T + h), T, h, w, bits, pattern)).to(dev)
    sink = torch.empty_like(codes)
    w5, w15 = TemporalFilter(window=5), TemporalFilter(window=15)
    return {"copy_": lambda: sink.copy_(codes),
            "window 5": lambda: w5(codes),
            "window 5 + stats": lambda: w5(codes, stats=True),
            "window 15": lambda: w15(codes)}, w5, codes


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for T, h, w, bits in SEQUENCES:
        for pattern in PATTERNS:
            variants, w5, codes = call_variants(T, h, w, bits, pattern, dev)
            name = f"{T} x {h}x{w} u{bits} {pattern}"
            st = w5(codes, stats=True)[1].cpu().numpy().view(np.uint32).astype(np.int64).sum(axis=0)
            print(f"{name}: valid {st[0]} rejected {st[1]} filled {st[2]} changed {st[3]}")
            for fn in variants.values():
                for _ in range(WARMUP):
                    fn()
            torch.cuda.synchronize(dev)
            times = {k: [] for k in variants}
            for _ in range(WINDOWS):
                for k, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(CALLS):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e3 / CALLS)
            floor = statistics.median(times["copy_"])
            for k, v in times.items():
                rows.append({"sequence": f"{T}x{h}x{w}", "bits": bits, "pattern": pattern, "variant": k, "us": v})
                print(f"{name} {k}: {spread(v)} us per call, {statistics.median(v) / floor:.2f} x the copy", flush=True)
    return rows


def run_kernels():
    dev = torch.device("cuda:0")
    for T, h, w, bits in SEQUENCES:
        for pattern in PATTERNS:
            for fn in call_variants(T, h, w, bits, pattern, dev)[0].values():
                for _ in range(200):
                    fn()
                torch.cuda.synchronize(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["calls", "kernels"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    rows = []
    if a.what == "kernels":
        run_kernels()
    else:
        rows = time_calls()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "what": a.what, "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
