"""Time per call of metrics.normal_errors next to metrics.depth_errors (edge evaluation on, r = 1) on the same planes.
Each figure is the median over WINDOWS windows of CALLS back-to-back calls, a window timed by two device events, after WARMUP calls
of every variant; the variants alternate window by window.  A call is the entry's memset plus its one kernel, enqueued from
Python: at the small size the host's enqueue rate is part of the figure.  The planes are a smooth surface with a nearer half, a
tenth of holes and a few codes of noise on the output, so most valid pixels have both normals and the histogram has many bins.

    python tools/time_normal_errors.py [--json FILE]
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
from codon_amd.register import Camera  # noqa: E402

WARMUP, WINDOWS, CALLS = 50, 30, 100
CASES = ((480, 640, 8), (1920, 2560, 16))
RADII = (2, 8)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    rows = []
    for H, W, bits in CASES:
        g = np.random.default_rng(bits)
        top = 255 if bits == 8 else 65535
        dt = np.uint8 if bits == 8 else np.uint16
        i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        z = top // 2 + (top // 50) * np.sin(0.02 * i + 0.1) * np.cos(0.015 * j)
        z = np.where(j > W // 2, z // 2, z)
        label = np.where(g.uniform(size=(H, W)) < 0.1, 0, np.clip(np.rint(z), 1, top))
        out = np.clip(label + g.integers(-(top // 1000) - 1, top // 1000 + 1, size=(H, W), endpoint=True), 1, top)
        label, out = torch.from_numpy(label.astype(dt)).to(dev), torch.from_numpy(out.astype(dt)).to(dev)
        cam = Camera(W, H, 0.9 * W, 0.9 * W, 0.5 * W - 0.25, 0.5 * H + 0.125)
        tol, T = max(2, top // 500), max(2, top // 50)
        variants = {"depth_errors edge r=1": lambda: metrics.depth_errors(label, out, thresholds=(1, 3), edge_threshold=T, edge_radius=1)}
        for r in RADII:
            variants[f"normal_errors R={r}"] = lambda r=r: metrics.normal_errors(label, out, cam, radius=r, tolerance=tol)
            variants[f"normal_errors R={r} + map"] = lambda r=r: metrics.normal_errors(label, out, cam, radius=r, tolerance=tol,
                                                                                     angle_map=True)
        words = metrics.normal_errors(label, out, cam, radius=2, tolerance=tol).cpu().numpy()[0]
        rep = metrics.normal_report(words)
        print(json.dumps({"size": f"{H}x{W}", "bits": bits, "compared": rep["normal_n"], "coverage": round(rep["normal_coverage"], 4),
                          "bins": int((words[:metrics.NORMAL_BINS] != 0).sum()), "mean_deg": round(rep["normal_mean"], 3)}), flush=True)
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
