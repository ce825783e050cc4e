"""What the undistortion of colour images costs, on the GPU: codon_amd.undistort.Undistortion's call beside the
bicubic baseline (upsample.bicubic_upsample_codes) writing a plane of the same size in ONE process, so that the bicubic launch is
the yardstick of a launch of that size on that box.  Legs alternate after a warm-up leg, and the spread of every leg is printed
beside the medians.

    python tools/time_undistort.py calls [--only NAME] [--json FILE]
                                            time per call for 480 x 640 grey and 1080 x 1920 grey and RGB under a barrel lens
                                            over a 56 degree field, one image and a batch of 8: device events around windows of
                                            back-to-back calls, enqueued from Python.  --only: one shape, e.g. 1080x1920x3
    python tools/time_undistort.py kernels  a few hundred calls of the same and nothing else: the run to trace
                                            (rocprofv3 --kernel-trace --stats -- python tools/time_undistort.py kernels)

The library with the staged window compiled out, for the same-box comparison of DESIGN 12.16:
    tools/ab_build.sh direct undistort.hip -DCODON_UD_STAGE=0
    CODON_AMD_LIB=$PWD/tools/probes/bin/libcodon_hip_direct.so python tools/time_undistort.py calls --only 1080x1920x3
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.register import Camera  # noqa: E402
from codon_amd.undistort import Undistortion  # noqa: E402
from codon_amd.upsample import bicubic_upsample_codes  # noqa: E402
from time_fill import spread  # noqa: E402

BARREL = (-0.3, 0.1, 1e-3, 1e-3, 0.0)
SHAPES = {"480x640x1": (480, 640, 1), "1080x1920x1": (1080, 1920, 1), "1080x1920x3": (1080, 1920, 3)}
BATCHES = (1, 8)
WARMUP, WINDOWS, CALLS = 50, 30, 100


def camera(h, w):
    f = 0.5 * w / math.tan(math.radians(28.0))                          # 56 degrees across the width
    return Camera(w, h, f, f, (w - 1) / 2 + 0.37, (h - 1) / 2 - 0.19, BARREL)


def call_variants(name, B, dev):
    h, w, c = SHAPES[name]
    g = np.random.default_rng(B + c)
    und = Undistortion(camera(h, w), device=dev)
    img = torch.from_numpy(g.integers(0, 256, size=(B, h, w, c) if c == 3 else (B, h, w), dtype=np.uint8)).to(dev)
    lr = torch.from_numpy(g.integers(1, 10000, size=(B, h // 4, w // 4)).astype(np.int16)).to(dev)
    return {"bicubic_upsample_codes": lambda: bicubic_upsample_codes(lr, 4), "undistort": lambda: und(img, c)}, und


def time_calls(only):
    dev = torch.device("cuda:0")
    rows = []
    for name in ([only] if only else SHAPES):
        for B in BATCHES:
            variants, und = call_variants(name, B, dev)
            print(f"{B} x {name}: {und.counts}")
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
                rows.append({"shape": name, "batch": B, "variant": k, "counts": und.counts, "us": v})
                print(f"{B} x {name} {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels(only):
    dev = torch.device("cuda:0")
    for name in ([only] if only else SHAPES):
        for B in BATCHES:
            for fn in call_variants(name, B, dev)[0].values():
                for _ in range(300):
                    fn()
                torch.cuda.synchronize(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["calls", "kernels"])
    ap.add_argument("--only", default=None, choices=list(SHAPES))
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    rows = []
    if a.what == "kernels":
        run_kernels(a.only)
    else:
        rows = time_calls(a.only)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "lib": os.environ.get("CODON_AMD_LIB", "in-tree"), "what": a.what,
                       "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
