"""What per-image range normalisation costs, on the GPU.  Everything runs in ONE process, so that the numbers of one
call can be compared with each other; loop legs alternate after a warm-up leg, and the spread of the repeated legs is printed
beside every median.

    python tools/time_stretch.py [--json FILE] [--skip-infer]
        calls   time per call of upsample.code_range, stretch_codes (with the range given) and unstretch_codes at 1x120x160,
                1x240x320 and 1x480x640, u8 and u16 codes: device events around windows of back-to-back calls enqueued from
                Python, beside infer.codes_to_input at the same low-resolution size (the launch that follows the stretch)
        infer   images/s of codon_amd.infer --lr-depth against --lr-depth --normalize on twelve 120x160 -> 480x640 pairs
                (x4, f16, random weights)
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd import CODONNet, infer, io  # noqa: E402
from codon_amd.upsample import code_range, stretch_codes, unstretch_codes  # noqa: E402

SIZES = ((120, 160), (240, 320), (480, 640))
WARMUP, WINDOWS, CALLS = 50, 20, 100


def spread(v):
    return f"{statistics.median(v):.4g} [{min(v):.4g} ... {max(v):.4g}]"


def lr_plane(g, h, w, top):
    """a scene in a fifth of the grid, 6 % holes"""
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.clip(np.rint((0.16 + 0.1 * np.sin(0.21 * yy) * np.cos(0.13 * xx)) * top), 1, top)
    c[g.uniform(size=(h, w)) < 0.06] = 0
    return c.astype(np.uint8 if top == 255 else np.uint16)


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for bits in (8, 16):
        top = 255 if bits == 8 else 65535
        for h, w in SIZES:
            plane = lr_plane(np.random.default_rng(bits), h, w, top)[None]
            codes = torch.from_numpy(plane.view(np.int16) if bits == 16 else plane).to(dev)
            lo_hi = code_range(codes)
            stretched = stretch_codes(codes, None, lo_hi)[0]
            variants = {"code_range": lambda: code_range(codes), "stretch_codes": lambda: stretch_codes(codes, None, lo_hi),
                        "unstretch_codes": lambda: unstretch_codes(stretched, lo_hi),
                        "codes_to_input": lambda: infer.codes_to_input(codes, 4, torch.float16)}
            if h * 4 > 1024:                                         # the x4 input of a 480x640 map is not a case of the loop
                del variants["codes_to_input"]
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
                rows.append({"shape": f"1x{h}x{w}", "bits": bits, "variant": k, "us": v})
                print(f"1x{h}x{w} u{bits} {k}: {spread(v)} us per call", flush=True)
    return rows


def time_infer(rounds=5, repeats=3, n=12, h=120, w=160, s=4):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = CODONNet().to(dev).to(torch.float16).eval()
    g = np.random.default_rng(5)
    with tempfile.TemporaryDirectory() as tmp:
        lrd, cd = os.path.join(tmp, "lr"), os.path.join(tmp, "color")
        os.makedirs(lrd)
        os.makedirs(cd)
        for i in range(n):
            io.write_gray(os.path.join(lrd, f"{i:02d}.png"), lr_plane(g, h, w, 255))
            io.write_gray(os.path.join(cd, f"{i:02d}.png"), g.integers(0, 256, size=(h * s, w * s)).astype(np.uint8))

        def leg(norm):
            k = t = 0.0
            for _ in range(repeats):
                r = infer.run_loop(m, dev, torch.float16, None, cd, None, None, emit=lambda s: None, lr_depth=lrd, scale=s,
                                   **({"normalize": True} if norm else {}))
                k, t = k + r["n"], t + r["seconds"]
            return k / t

        leg(False), leg(True)                                        # warm-up legs
        off, on = [], []
        for _ in range(rounds):
            off.append(leg(False))
            on.append(leg(True))
    print(f"infer, {n} pairs {h}x{w} -> {h * s}x{w * s}, f16: --lr-depth {spread(off)} images/s, --lr-depth --normalize {spread(on)} "
          f"images/s, medians {100 * (statistics.median(on) / statistics.median(off) - 1):+.2f} %", flush=True)
    return [{"images_per_s_off": off, "images_per_s_on": on}]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-infer", action="store_true")
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    rows = {"calls": time_calls()}
    if not a.skip_infer:
        rows["infer"] = time_infer()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
