"""What the guidance-aware hole filler costs, on the GPU, beside the plain filler in the same process.  Legs
alternate after a warm-up leg, and the spread of every leg is printed beside the medians.

    python tools/time_guided_fill.py calls [--json FILE]   time per call of upsample.fill_holes_guided beside upsample.fill_holes at
                                                           16x32x32 (x4, one launch: a training batch of crops), 1x120x160 and
                                                           1x93x116 (x4, three launches), u8 codes: device events around windows of
                                                           back-to-back calls, enqueued from Python
    python tools/time_guided_fill.py infer [--json FILE]   images/s of codon_amd.infer --lr-depth --fill-holes against the same plus
                                                           --fill-guided on twelve holey 93x116 -> 372x464 pairs (x4, f16, random
                                                           weights)
    python tools/time_guided_fill.py all   [--json FILE]   both, in one process
    python tools/time_guided_fill.py kernels               a few hundred calls of the three shapes and nothing else: the run to
                                                           trace (rocprofv3 --kernel-trace --stats -- python
                                                           tools/time_guided_fill.py kernels); also prints the host's own time
                                                           per call, enqueue only
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd import CODONNet, infer  # noqa: E402
from codon_amd.upsample import fill_holes, fill_holes_guided  # noqa: E402
from time_fill import lr_plane, spread, write_infer_set  # noqa: E402

CALL_CASES = ((16, 32, 32, 4), (1, 120, 160, 4), (1, 93, 116, 4))   # B, h, w, scale
WARMUP, WINDOWS, CALLS = 50, 30, 100


def call_variants(B, h, w, s, dev):
    g = np.random.default_rng(h)
    codes = torch.from_numpy(np.stack([lr_plane(g, h, w, 255, True) for _ in range(B)])).to(dev)
    guide = torch.from_numpy(g.integers(0, 256, size=(B, h * s, w * s), dtype=np.uint8)).to(dev)
    return {"fill_holes": lambda: fill_holes(codes), "fill_holes_guided": lambda: fill_holes_guided(codes, guide, s)}


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for B, h, w, s in CALL_CASES:
        variants = call_variants(B, h, w, s, dev)
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
            rows.append({"shape": f"{B}x{h}x{w}", "scale": s, "variant": k, "us": v})
            print(f"{B}x{h}x{w} x{s} u8 {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels():
    import time
    dev = torch.device("cuda:0")
    for B, h, w, s in CALL_CASES:
        variants = call_variants(B, h, w, s, dev)
        for k, fn in variants.items():
            for _ in range(50):
                fn()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for _ in range(300):
                fn()
            t1 = time.perf_counter()
            torch.cuda.synchronize(dev)
            print(f"{B}x{h}x{w} x{s} u8 {k}: host {1e6 * (t1 - t0) / 300:.2f} us per call to enqueue", flush=True)
    return []


def time_infer(rounds=5, repeats=4):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = CODONNet().to(dev).to(torch.float16).eval()
    with tempfile.TemporaryDirectory() as tmp:
        lrd, cd = write_infer_set(os.path.join(tmp, "holey"), True)

        def leg(guided):
            n = t = 0.0
            for _ in range(repeats):                                 # twelve images are a few tens of milliseconds: repeat the loop
                r = infer.run_loop(m, dev, torch.float16, None, cd, None, None, emit=lambda s: None, lr_depth=lrd, scale=4,
                                   fill_holes=True, **({"fill_guided": True} if guided else {}))
                n, t = n + r["n"], t + r["seconds"]
            return n / t

        leg(False), leg(True)                                        # warm-up legs
        off, on = [], []
        for _ in range(rounds):
            off.append(leg(False))
            on.append(leg(True))
    print(f"infer, holey files: --lr-depth --fill-holes {spread(off)} images/s, + --fill-guided {spread(on)} images/s, "
          f"medians {100 * (statistics.median(on) / statistics.median(off) - 1):+.2f} %", flush=True)
    return [{"files": "holey", "images_per_s_plain": off, "images_per_s_guided": on}]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["calls", "infer", "all", "kernels"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    if a.what == "kernels":
        run_kernels()
    rows = (time_calls() if a.what in ("calls", "all") else []) + (time_infer() if a.what in ("infer", "all") else [])
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "what": a.what, "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
