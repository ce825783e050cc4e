"""What the pull-push hole filler costs, on the GPU.  Legs alternate in ONE process after a warm-up leg, and the
spread of the repeated baseline legs is printed beside every difference.

    python tools/time_fill.py infer   [--json FILE]   images/s of codon_amd.infer --lr-depth against --lr-depth --fill-holes on
                                                      twelve 93x116 -> 372x464 pairs (x4, f16, random weights), hole-free files
                                                      and holey ones
    python tools/time_fill.py calls   [--json FILE]   time per call of upsample.fill_holes beside infer.codes_to_input (the launch
                                                      that follows it) at 1x93x116 u8 (x4) and 8x120x160 u16 (x16): device
                                                      events around windows of back-to-back calls, enqueued from Python
    python tools/time_fill.py train   [--json FILE]   a training step at the CLI defaults (x4, crop 128, batch 16, bf16) with
                                                      --degrade-holes --mask-holes against the same plus --fill-holes
    python tools/time_fill.py kernels                 a few hundred calls of the same two shapes and nothing else: the run to
                                                      trace (rocprofv3 --kernel-trace --stats -- python tools/time_fill.py kernels)
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
from codon_amd import CODONNet, infer, io, train  # noqa: E402
from codon_amd.upsample import fill_holes  # noqa: E402

CALL_CASES = ((1, 93, 116, 8, 4), (8, 120, 160, 16, 16))            # B, h, w, code bits, scale
WARMUP, WINDOWS, CALLS = 50, 30, 100


def spread(v):
    return f"{statistics.median(v):.4g} [{min(v):.4g} ... {max(v):.4g}]"


def lr_plane(g, h, w, top, holes):
    yy, xx = np.mgrid[0:h, 0:w]
    c = np.clip(np.rint((0.5 + 0.4 * np.sin(0.21 * yy) * np.cos(0.13 * xx)) * top), 1, top)
    if holes:                                                       # 6 % isolated holes and three blobs wider than the cubic's support
        c[g.uniform(size=(h, w)) < 0.06] = 0
        for _ in range(3):
            y0, x0 = int(g.integers(0, h - 12)), int(g.integers(0, w - 16))
            c[y0:y0 + 12, x0:x0 + 16] = 0
    return c.astype(np.uint8 if top == 255 else np.uint16)


def write_infer_set(root, holes, n=12, h=93, w=116, s=4):
    g = np.random.default_rng(5)
    lrd, cd = os.path.join(root, "lr"), os.path.join(root, "color")
    os.makedirs(lrd)
    os.makedirs(cd)
    for i in range(n):
        io.write_gray(os.path.join(lrd, f"{i:02d}.png"), lr_plane(g, h, w, 255, holes))
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g.integers(0, 256, size=(h * s, w * s)).astype(np.uint8))
    return lrd, cd


def time_infer(rounds=5, repeats=4):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    m = CODONNet().to(dev).to(torch.float16).eval()
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for holes in (False, True):
            lrd, cd = write_infer_set(os.path.join(tmp, "holey" if holes else "dense"), holes)

            def leg(fill):
                n = t = 0.0
                for _ in range(repeats):                             # twelve images are a few tens of milliseconds: repeat the loop
                    r = infer.run_loop(m, dev, torch.float16, None, cd, None, None, emit=lambda s: None, lr_depth=lrd, scale=4,
                                       **({"fill_holes": True} if fill else {}))
                    n, t = n + r["n"], t + r["seconds"]
                return n / t

            leg(False), leg(True)                                    # warm-up legs
            off, on = [], []
            for _ in range(rounds):
                off.append(leg(False))
                on.append(leg(True))
            row = {"files": "holey" if holes else "hole-free", "images_per_s_off": off, "images_per_s_on": on}
            rows.append(row)
            print(f"infer, {row['files']} files: --lr-depth {spread(off)} images/s, --lr-depth --fill-holes {spread(on)} images/s, "
                  f"medians {100 * (statistics.median(on) / statistics.median(off) - 1):+.2f} %", flush=True)
    return rows


def call_variants(B, h, w, bits, s, dev):
    g = np.random.default_rng(bits)
    top = 255 if bits == 8 else 65535
    planes = np.stack([lr_plane(g, h, w, top, True) for _ in range(B)])
    codes = torch.from_numpy(planes.view(np.int16) if bits == 16 else planes).to(dev)
    tdt = torch.float16 if bits == 8 else torch.bfloat16
    return {"fill_holes": lambda: fill_holes(codes), "codes_to_input": lambda: infer.codes_to_input(codes, s, tdt)}


def time_calls():
    dev = torch.device("cuda:0")
    rows = []
    for B, h, w, bits, s in CALL_CASES:
        variants = call_variants(B, h, w, bits, s, dev)
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
            rows.append({"shape": f"{B}x{h}x{w}", "bits": bits, "variant": k, "us": v})
            print(f"{B}x{h}x{w} u{bits} {k}: {spread(v)} us per call", flush=True)
    return rows


def run_kernels():
    dev = torch.device("cuda:0")
    for B, h, w, bits, s in CALL_CASES:
        variants = call_variants(B, h, w, bits, s, dev)
        for _ in range(300):
            for fn in variants.values():
                fn()
        torch.cuda.synchronize(dev)
    return []


def write_train_set(root, n=4, h=480, w=640):
    g = np.random.default_rng(7)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd)
    os.makedirs(cd)
    for i in range(n):
        yy, xx = np.mgrid[0:h, 0:w]
        d = np.clip(127.5 + 100 * np.sin(0.011 * yy + 0.3 * i) * np.cos(0.007 * xx), 1, 255).astype(np.uint8)
        d[g.uniform(size=(h, w)) < 0.05] = 0
        for _ in range(40):                                         # blobs that survive the x4 reduction
            y0, x0 = int(g.integers(0, h - 40)), int(g.integers(0, w - 40))
            d[y0:y0 + 40, x0:x0 + 40] = 0
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), np.clip(d.astype(int) + g.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8))
    return dd, cd


def time_train(rounds=3, steps=60):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        dd, cd = write_train_set(tmp)
        ts = train.TrainSet(dd, cd, "cuda:0", crop=128)

        def leg(fill):
            torch.manual_seed(0)
            r = train.fit(CODONNet().cuda(), ts, steps, scale=4, seed=3, log_every=steps, emit=lambda s: None, time_synth=True,
                          mask_holes=True, degrade_holes=True, **({"fill_holes": True} if fill else {}))
            return statistics.median(r["step_ms"][10:]), 1e3 * statistics.median(r["synth_ms"][10:])

        leg(False), leg(True)                                        # warm-up legs
        off, on = [], []
        for _ in range(rounds):
            off.append(leg(False))
            on.append(leg(True))
        for name, k in (("step ms", 0), ("synthesize us", 1)):
            a, b = [v[k] for v in off], [v[k] for v in on]
            rows.append({"what": name, "off": a, "on": b})
            print(f"train {name}: --degrade-holes --mask-holes {spread(a)}, + --fill-holes {spread(b)}", flush=True)
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["infer", "calls", "train", "kernels"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    rows = {"infer": time_infer, "calls": time_calls, "train": time_train, "kernels": run_kernels}[a.what]()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "what": a.what, "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
