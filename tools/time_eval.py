"""Time per call of metrics.depth_errors next to metrics.masked_sqerr_dev on the same planes.  Each figure is the
median over WINDOWS windows of CALLS back-to-back calls, a window timed by two device events, after WARMUP calls of every
variant; the variants alternate window by window.  A call is the entry's memset plus its one kernel, enqueued from Python: at
the small size the host's enqueue rate is part of the figure.

    python tools/time_eval.py [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd import metrics  # noqa: E402

WARMUP, WINDOWS, CALLS = 50, 30, 100
CASES = ((480, 640, 8), (1920, 2560, 16))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    rows = []
    for H, W, bits in CASES:
        g = np.random.default_rng(bits)
        top, step = (255, 60) if bits == 8 else (65535, 12000)
        dt = np.uint8 if bits == 8 else np.uint16
        label = (40 + step * g.integers(0, 4, size=(H // 16 + 1, W // 16 + 1))).repeat(16, 0).repeat(16, 1)[:H, :W]
        label = np.where(g.uniform(size=(H, W)) < 0.1, 0, label)
        out = np.clip(label + g.integers(-6, 6, size=(H, W), endpoint=True), 0, top)
        label, out = torch.from_numpy(label.astype(dt)).to(dev), torch.from_numpy(out.astype(dt)).to(dev)
        thr, T = ((0, 1, 3, 5), 20) if bits == 8 else ((0, 200, 600, 1000), 4000)
        sqerr = metrics.masked_sqerr_dev if bits == 8 else metrics.masked_sqerr_u16_dev
        variants = {
            "masked_sqerr": lambda: sqerr(label, out),
            "depth_errors edge off": lambda: metrics.depth_errors(label, out, thresholds=thr),
            "depth_errors r=0": lambda: metrics.depth_errors(label, out, thresholds=thr, edge_threshold=T, edge_radius=0),
            "depth_errors r=8": lambda: metrics.depth_errors(label, out, thresholds=thr, edge_threshold=T, edge_radius=8),
            "depth_errors r=8 + maps": lambda: metrics.depth_errors(label, out, thresholds=thr, edge_threshold=T, edge_radius=8,
                                                                    error_map=True, region_map=True),
        }
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
            row = {"size": f"{H}x{W}", "bits": bits, "variant": k, "us_median": round(statistics.median(v), 2),
                   "us_min": round(min(v), 2), "us_max": round(max(v), 2), "windows": WINDOWS, "calls": CALLS}
            rows.append(row)
            print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
