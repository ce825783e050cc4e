"""What the outlier rejection of sensor depth maps costs, on the GPU: codon_amd.clean.Cleaner's call beside the
bicubic baseline (upsample.bicubic_upsample_codes) writing a plane of the same size in ONE process, so that the bicubic launch is
the yardstick of a launch of that size on that box.  Legs alternate after a warm-up leg, and the spread of every leg is printed
beside the medians.

    python tools/time_clean.py calls [--json FILE]   time per call, u16 codes, for a 424 x 512 and a 576 x 640 sensor, one image
                                                     and a batch of 8, a noisy scene with 5 % holes and the constant plane (one
                                                     component over everything: the contended path of the count launch), with
                                                     and without statistics, and with rule 2 off: device events around windows
                                                     of back-to-back calls, enqueued from Python
    python tools/time_clean.py kernels               a few hundred calls of the same and nothing else: the run to trace
                                                     (rocprofv3 --kernel-trace --stats -- python tools/time_clean.py kernels)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.clean import Cleaner  # noqa: E402
from codon_amd.upsample import bicubic_upsample_codes  # noqa: E402
from time_fill import spread  # noqa: E402

SENSORS = ((424, 512), (576, 640))
BATCHES = (1, 8)
PATTERNS = ("scene", "constant")
WARMUP, WINDOWS, CALLS = 50, 30, 100


def scene(g, B, h, w):
    """B planes of millimetres: a smooth background 1.5 - 4 m with +- 3 codes of noise, a nearer box with a ring of mixed
    measurements around it, 5 % holes"""
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.rint(2750 + 1250 * np.sin(0.011 * yy) * np.cos(0.007 * xx)).astype(np.int64)
    planes = []
    for _ in range(B):
        p = c + g.integers(-3, 4, size=(h, w))
        y0, x0 = int(g.integers(1, h // 2)), int(g.integers(1, w // 2))
        box = p[y0 - 1:y0 + h // 3 + 1, x0 - 1:x0 + w // 3 + 1]
        box[...] = np.rint(900 + g.uniform(0.15, 0.85, size=box.shape) * (box - 900))
        p[y0:y0 + h // 3, x0:x0 + w // 3] = 900 + g.integers(-3, 4, size=(h // 3, w // 3))
        p[g.uniform(size=(h, w)) < 0.05] = 0
        planes.append(p)
    return np.stack(planes).astype(np.uint16)


def call_variants(h, w, B, pattern, dev):
    g = np.random.default_rng(B + h)
    plane = scene(g, B, h, w) if pattern == "scene" else np.full((B, h, w), 2750, dtype=np.uint16)
    codes = torch.from_numpy(plane.view(np.int16)).to(dev)
    lr = torch.from_numpy(scene(g, B, h // 4, w // 4).view(np.int16)).to(dev)
    clean, rule1 = Cleaner(), Cleaner(min_region=0)
    return {"bicubic_upsample_codes": lambda: bicubic_upsample_codes(lr, 4),
            "clean": lambda: clean(codes),
            "clean+stats": lambda: clean(codes, stats=True),
            "clean rule 2 off": lambda: rule1(codes)}, clean, codes


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for h, w in SENSORS:
        for B in BATCHES:
            for pattern in PATTERNS:
                variants, clean, codes = call_variants(h, w, B, pattern, dev)
                name = f"{B} x {h}x{w} {pattern}"
                st = clean(codes, stats=True)[1].cpu().numpy().view(np.uint32).sum(axis=0)
                print(f"{name}: valid {st[0]} flying {st[1]} speckle {st[2]} regions {st[3]}")
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
                for k, v in times.items():
                    rows.append({"sensor": f"{h}x{w}", "batch": B, "pattern": pattern, "variant": k, "us": v})
                    print(f"{name} {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels():
    dev = torch.device("cuda:0")
    for h, w in SENSORS:
        for B in BATCHES:
            for pattern in PATTERNS:
                for fn in call_variants(h, w, B, pattern, dev)[0].values():
                    for _ in range(300):
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
