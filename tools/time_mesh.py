"""What the triangle meshes cost, on the GPU: codon_amd.cloud.triangulate's call beside Unprojection's
(codon_cloud_points, with and without normals) on the same planes in ONE process, for context; there is no pass/fail bar, because
nothing exists to measure against.  Legs alternate after a warm-up leg, and the spread of every leg is printed beside the medians:
us per call, median [min ... max] of 30 windows of 100 calls (20 windows of 20 on the large plane).

    python tools/time_mesh.py calls [--json FILE]   time per call and achieved GB/s for a 480 x 640 plane of u8 codes and a
                                                    1920 x 2560 plane of u16 codes, one image, a smooth scene with 5 % holes:
                                                    device events around windows of back-to-back calls, enqueued from Python.
                                                    GB/s counts what the six launches move by their text: the codes read four
                                                    times (vertex count, index, face count, face emit), the int32 index plane
                                                    written once and read once, the 13-byte records written once
    python tools/time_mesh.py kernels               a few hundred calls of the same and nothing else: the run to trace
                                                    (rocprofv3 --kernel-trace --stats -- python tools/time_mesh.py kernels)
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.cloud import FACE_REC, Unprojection, triangulate  # noqa: E402
from codon_amd.register import Camera  # noqa: E402
from time_cloud import scene  # noqa: E402
from time_fill import spread  # noqa: E402

# (h, w, bits, warm-up calls, windows, calls per window)
MAPS = ((480, 640, 8, 50, 30, 100), (1920, 2560, 16, 10, 20, 20))


def plane(h, w, bits):
    """time_cloud's scene: millimetres as u16 codes, or a sixteenth of them as u8 codes"""
    c = scene(np.random.default_rng(h), h, w)
    return c if bits == 16 else np.minimum(c // 16, 255).astype(np.uint8)


def call_variants(h, w, bits, dev):
    c = plane(h, w, bits)
    codes = torch.from_numpy(c.view(np.int16) if bits == 16 else c).to(dev)
    cam = Camera(w, h, 0.9 * w, 0.9 * w, (w - 1) / 2.0, (h - 1) / 2.0)
    full, xyz = Unprojection(cam), Unprojection(cam, normals=False)
    return {"cloud xyz": lambda: xyz(codes), "cloud xyz+normals": lambda: full(codes), "mesh": lambda: triangulate(codes)}, codes


def moved_bytes(h, w, bits, faces):
    return 4 * h * w * (bits // 8) + 2 * 4 * h * w + faces * FACE_REC


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for h, w, bits, warmup, windows, calls in MAPS:
        variants, codes = call_variants(h, w, bits, dev)
        name = f"{h}x{w} u{bits}"
        faces = int(triangulate(codes).counts.cpu().numpy().view(np.uint32)[0])
        print(f"{name}: faces {faces} of {2 * (h - 1) * (w - 1)}, {faces * FACE_REC / 1e6:.1f} MB of records")
        for fn in variants.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize(dev)
        times = {k: [] for k in variants}
        for _ in range(windows):
            for k, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(calls):
                    fn()
                e1.record()
                e1.synchronize()
                times[k].append(e0.elapsed_time(e1) * 1e3 / calls)
        for k, v in times.items():
            row = {"map": name, "variant": k, "us": v}
            line = f"{name} {k}: {spread(v)} us per call"
            if k == "mesh":
                row["bytes"] = moved_bytes(h, w, bits, faces)
                row["gb_per_s"] = row["bytes"] / (float(np.median(v)) * 1e-6) / 1e9
                line += f", {row['bytes'] / 1e6:.1f} MB moved: {row['gb_per_s']:.0f} GB/s"
            rows.append(row)
            print(line, flush=True)
    return rows


def run_kernels():
    dev = torch.device("cuda:0")
    for h, w, bits, *_ in MAPS:
        for fn in call_variants(h, w, bits, dev)[0].values():
            for _ in range(300 if h < 1000 else 40):
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
