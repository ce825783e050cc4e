"""What the depth registration costs, on the GPU: codon_amd.register.Registration's call beside the bicubic
baseline (upsample.bicubic_upsample_codes) writing a plane of about the same size in ONE process, so that the bicubic launch is
the yardstick of a launch of that size on that box.  Legs alternate after a warm-up leg, and the spread of every leg is printed
beside the medians.

    python tools/time_register.py calls [--json FILE]   time per call, u16 codes, for a 512 x 424 sensor onto 480 x 270 (a 1920 x 1080
                                                        colour image at scale 4) and a 640 x 576 sensor onto 1920 x 1080 (scale 1),
                                                        one image and a batch of 8: device events around windows of back-to-back
                                                        calls, enqueued from Python
    python tools/time_register.py kernels               a few hundred calls of the same and nothing else: the run to trace
                                                        (rocprofv3 --kernel-trace --stats -- python tools/time_register.py kernels)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.register import Calibration, Camera, Registration  # noqa: E402
from codon_amd.upsample import bicubic_upsample_codes  # noqa: E402
from time_fill import spread  # noqa: E402

# name -> (depth camera, colour camera, scale, the bicubic yardstick's low-resolution plane at x4)
RIGS = {
    "424x512->270x480 s4": (Camera(512, 424, 365.0, 365.0, 255.5, 211.5, (0.09, -0.27, 0.0, 0.0, 0.09)),
                            Camera(1920, 1080, 1060.0, 1060.0, 959.5, 539.5), 4, (67, 120)),
    "576x640->1080x1920 s1": (Camera(640, 576, 504.0, 504.0, 319.5, 287.5, (0.1, -0.05, 1e-4, -1e-4, 0.0)),
                              Camera(1920, 1080, 915.0, 915.0, 959.5, 539.5), 1, (270, 480)),
}
ROT = [[0.99995, -0.00999983, 0.0], [0.00999983, 0.99995, 0.0], [0.0, 0.0, 1.0]]       # a roll of 0.01 rad
BATCHES = (1, 8)
WARMUP, WINDOWS, CALLS = 50, 30, 100


def scene(g, B, h, w):
    """B planes of millimetres: a smooth background 1.5 - 4 m, a nearer box, 5 % holes"""
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.rint(2750 + 1250 * np.sin(0.011 * yy) * np.cos(0.007 * xx)).astype(np.int64)
    planes = []
    for _ in range(B):
        p = c.copy()
        y0, x0 = int(g.integers(0, h // 2)), int(g.integers(0, w // 2))
        p[y0:y0 + h // 3, x0:x0 + w // 3] = 900
        p[g.uniform(size=(h, w)) < 0.05] = 0
        planes.append(p)
    return np.stack(planes).astype(np.uint16)


def call_variants(name, B, dev):
    depth, color, s, (lh, lw) = RIGS[name]
    g = np.random.default_rng(B + s)
    reg = Registration(Calibration(depth, color, ROT, (0.052, 0.001, -0.003)), s, 0.001, device=dev)
    codes = torch.from_numpy(scene(g, B, depth.height, depth.width).view(np.int16)).to(dev)
    lr = torch.from_numpy(scene(g, B, lh, lw).view(np.int16)).to(dev)
    return {"bicubic_upsample_codes": lambda: bicubic_upsample_codes(lr, 4),
            "register": lambda: reg(codes),
            "register+stats": lambda: reg(codes, stats=True)}, reg, codes


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for name in RIGS:
        for B in BATCHES:
            variants, reg, codes = call_variants(name, B, dev)
            st = reg(codes, stats=True)[1].cpu().numpy().view(np.uint32).sum(axis=0)
            print(f"{B} x {name}: valid {st[0]} outside {st[1]} dropped {st[2]} filled {st[3]} of {B * reg.out_size[0] * reg.out_size[1]}")
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
                rows.append({"rig": name, "batch": B, "variant": k, "us": v})
                print(f"{B} x {name} {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels():
    dev = torch.device("cuda:0")
    for name in RIGS:
        for B in BATCHES:
            for fn in call_variants(name, B, dev)[0].values():
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
