"""What the classical baselines cost, on the GPU: joint bilateral upsampling beside the launch that builds the
network's input (infer.codes_to_input, fp32) and beside the bicubic baseline (upsample.bicubic_upsample_codes) at the same shapes in
ONE process, so that the bicubic launch is the yardstick on that box.  Legs alternate after a warm-up leg, and the spread of every
leg is printed beside the medians.

    python tools/time_jbu.py calls [--json FILE]   time per call at 1x120x160 x4 u8, 8x120x160 x4 u16 and 1x120x160 x16 u16, holey
                                                   planes: device events around windows of back-to-back calls, enqueued from Python
    python tools/time_jbu.py kernels               a few hundred calls of the three shapes and nothing else: the run to trace
                                                   (rocprofv3 --kernel-trace --stats -- python tools/time_jbu.py kernels); also
                                                   prints the host's own time per call, enqueue only
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd import infer  # noqa: E402
from codon_amd.upsample import bicubic_upsample_codes, joint_bilateral_upsample  # noqa: E402
from time_fill import lr_plane, spread  # noqa: E402

CALL_CASES = ((1, 120, 160, 4, 8), (8, 120, 160, 4, 16), (1, 120, 160, 16, 16))   # B, h, w, scale, code bits
WARMUP, WINDOWS, CALLS = 50, 30, 100


def call_variants(B, h, w, s, bits, dev):
    g = np.random.default_rng(h + s)
    top = 255 if bits == 8 else 65535
    planes = np.stack([lr_plane(g, h, w, top, True) for _ in range(B)])
    codes = torch.from_numpy(planes.view(np.int16) if bits == 16 else planes).to(dev)
    guide = torch.from_numpy(g.integers(0, 256, size=(B, h * s, w * s), dtype=np.uint8)).to(dev)
    return {"codes_to_input_f32": lambda: infer.codes_to_input(codes, s, torch.float32),
            "bicubic_upsample_codes": lambda: bicubic_upsample_codes(codes, s),
            "joint_bilateral_upsample": lambda: joint_bilateral_upsample(codes, guide, s)}


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for B, h, w, s, bits in CALL_CASES:
        variants = call_variants(B, h, w, s, bits, dev)
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
            rows.append({"shape": f"{B}x{h}x{w}", "scale": s, "bits": bits, "variant": k, "us": v})
            print(f"{B}x{h}x{w} x{s} u{bits} {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels():
    import time
    dev = torch.device("cuda:0")
    for B, h, w, s, bits in CALL_CASES:
        for k, fn in call_variants(B, h, w, s, bits, dev).items():
            for _ in range(50):
                fn()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(300):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize(dev)
            print(f"{B}x{h}x{w} x{s} u{bits} {k}: host {1e6 * (t1 - t0) / 300:.2f} us per call to enqueue", flush=True)


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
