"""What the point clouds with normals cost, on the GPU: codon_amd.cloud.Unprojection's call beside the bicubic
baseline (upsample.bicubic_upsample_codes) writing a plane of the same size in ONE process, so that the bicubic launch is the
yardstick of a launch of that size on that box.  Legs alternate after a warm-up leg, and the spread of every leg is printed beside
the medians: us per call, median [min ... max] of 30 windows of 100 calls.

    python tools/time_cloud.py calls [--json FILE]   time per call, u16 codes, for a 480 x 640 and a 1080 x 1920 map, one image,
                                                     a smooth scene with 5 % holes: the four record forms, the full form with the
                                                     normal map, and R = 8: device events around windows of back-to-back calls,
                                                     enqueued from Python
    python tools/time_cloud.py kernels               a few hundred calls of the same and nothing else: the run to trace
                                                     (rocprofv3 --kernel-trace --stats -- python tools/time_cloud.py kernels)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.cloud import Unprojection  # noqa: E402
from codon_amd.register import Camera  # noqa: E402
from codon_amd.upsample import bicubic_upsample_codes  # noqa: E402
from time_fill import spread  # noqa: E402

MAPS = ((480, 640), (1080, 1920))
WARMUP, WINDOWS, CALLS = 50, 30, 100


def scene(g, h, w):
    """A plane of millimetres: a smooth surface 1.5 - 4 m with +- 3 codes of noise, a nearer box, 5 % holes"""
    yy, xx = np.mgrid[0:h, 0:w]
    p = np.rint(2750 + 1250 * np.sin(0.011 * yy) * np.cos(0.007 * xx)).astype(np.int64) + g.integers(-3, 4, size=(h, w))
    p[h // 4:h // 4 + h // 3, w // 3:w // 3 + w // 3] = 900 + g.integers(-3, 4, size=(h // 3, w // 3))
    p[g.uniform(size=(h, w)) < 0.05] = 0
    return p[None].astype(np.uint16)


def call_variants(h, w, dev):
    g = np.random.default_rng(h)
    codes = torch.from_numpy(scene(g, h, w).view(np.int16)).to(dev)
    lr = torch.from_numpy(scene(g, h // 4, w // 4).view(np.int16)).to(dev)
    rgb = torch.from_numpy(g.integers(0, 256, size=(1, h, w, 3), dtype=np.uint8)).to(dev)
    cam = Camera(w, h, 0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    full, xyz, far = Unprojection(cam), Unprojection(cam, normals=False), Unprojection(cam, radius=8)
    return {"bicubic_upsample_codes": lambda: bicubic_upsample_codes(lr, 4),
            "cloud xyz": lambda: xyz(codes),
            "cloud xyz+rgb": lambda: xyz(codes, rgb),
            "cloud xyz+normals": lambda: full(codes),
            "cloud xyz+normals+rgb": lambda: full(codes, rgb),
            "cloud xyz+normals+rgb+map": lambda: full(codes, rgb, normal_map=True),
            "cloud xyz+normals+rgb R=8": lambda: far(codes, rgb)}, full, codes


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for h, w in MAPS:
        variants, full, codes = call_variants(h, w, dev)
        name = f"{h}x{w}"
        st = full(codes).counts.cpu().numpy().view(np.uint32)[0]
        print(f"{name}: points {st[0]} of {h * w}, normals {st[1]}")
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
            rows.append({"map": name, "variant": k, "us": v})
            print(f"{name} {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels():
    dev = torch.device("cuda:0")
    for h, w in MAPS:
        for fn in call_variants(h, w, dev)[0].values():
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
