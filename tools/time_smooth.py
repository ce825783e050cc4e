"""What the spatial smoothing of a depth map costs, on the GPU, in ONE process: codon_amd.smooth.Smoother's call beside
a `copy_` of the same bytes (every code read once and written once: the floor of the filter's bytes, and the yardstick of that
box), beside codon_amd.clean.Cleaner with rule 2 off on the same plane (the other tile-plus-halo filter of the sensor chain, a 3 x 3
link count), and beside P calls of passes=1 -- the unfused form of the same result, which is what decides the fusion rule of
csrc/launch_rules.h.  Legs alternate after a warm-up leg, and the spread of every leg is printed beside the medians.

    python tools/time_smooth.py calls [--json FILE]   424 x 512 u16, 480 x 640 u8 and 1920 x 2560 u16 planes of a noisy slanted scene
                                                      with 5 % holes, at the defaults (radius 2, passes 2) and at radius 4 with
                                                      passes 3; statistics at the defaults
    python tools/time_smooth.py rule [--json FILE]    every radius 1..4 at passes 2 and 3 on the u16 planes: the call as the
                                                      library's rule launches it (its plan is printed), the same passes as a call
                                                      of 2 and a call of 1, and as P calls of 1.  A library built with
                                                      -DCODON_SMOOTH_FUSE_ALL (make EXTRA=...) launches every call fused: the two
                                                      builds together are the measurement the rule rests on
    python tools/time_smooth.py kernels               a few hundred calls of the defaults and nothing else: the run to trace
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from codon_amd.clean import Cleaner  # noqa: E402
from codon_amd.smooth import Smoother, plan  # noqa: E402
from time_fill import spread  # noqa: E402

PLANES = ((424, 512, 16), (480, 640, 8), (1920, 2560, 16))           # h, w, code bits
PARAMS = ((2, 2), (4, 3))                                            # radius, passes
WARMUP, WINDOWS, CALLS = 10, 12, 20


def plane(g, h, w, bits):
    """A slanted background and a steeper slanted block in front of it, +- 12 codes (u16, top 10000) or +- 3 (u8) of noise, 5 % holes"""
    yy, xx = np.mgrid[0:h, 0:w]
    top, noise = (10000, 12) if bits == 16 else (255, 3)
    v = 60.0 + 100.0 * xx / w + 50.0 * yy / h
    v = np.where((yy > h // 5) & (yy < 3 * h // 4) & (xx > w // 4) & (xx < 3 * w // 4), 150.0 + 60.0 * (xx - w // 4) / w, v) * (top / 255.0)
    c = np.clip(np.rint(v + g.uniform(-noise, noise, size=(h, w))), 1, top)
    c[g.uniform(size=(h, w)) < 0.05] = 0
    return (c.astype(np.uint8) if bits == 8 else c.astype(np.uint16).view(np.int16)), (None if bits == 8 else top)


def in_turn(*fs):
    """the calls one after the other, each on the result of the one before"""
    def run(codes, dm):
        for f in fs:
            codes = f(codes, dm)
        return codes
    return run


def measure(name, variants, rows, extra):
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
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
    floor = statistics.median(times["copy_"])
    for k, v in times.items():
        rows.append(dict(extra, variant=k, us=v))
        print(f"{name} {k}: {spread(v)} us per call, {statistics.median(v) / floor:.2f} x the copy", flush=True)


def time_calls(dev):
    rows = []
    for h, w, bits in PLANES:
        a, dm = plane(np.random.default_rng(h), h, w, bits)
        codes = torch.from_numpy(a).to(dev)
        sink = torch.empty_like(codes)
        flying = Cleaner(min_region=0)
        variants = {"copy_": lambda: sink.copy_(codes), "clean, rule 2 off": lambda: flying(codes, dm)}
        for radius, passes in PARAMS:
            f, one = Smoother(radius, passes), Smoother(radius, 1)
            p = plan(radius, passes)
            tag = f"radius {radius} passes {passes}"
            variants[f"{tag} ({p['launches']} launch(es), {p['fused']} fused)"] = lambda f=f: f(codes, dm)
            variants[f"{tag} as {passes} calls of passes=1"] = lambda one=one, passes=passes: in_turn(*[one] * passes)(codes, dm)
            if (radius, passes) == PARAMS[0]:
                variants[f"{tag} + stats"] = lambda f=f: f(codes, dm, stats=True)
                st = f(codes, dm, stats=True)[1].cpu().numpy().view(np.uint32)[0]
                print(f"{h}x{w} u{bits}: valid {st[0]} changed {st[1]} alone {st[2]} max {st[3]}")
        measure(f"{h}x{w} u{bits}", variants, rows, dict(plane=f"{h}x{w}", bits=bits))
    return rows


def time_rule(dev):
    rows = []
    for h, w, bits in PLANES:
        if bits != 16:
            continue
        a, dm = plane(np.random.default_rng(h), h, w, bits)
        codes = torch.from_numpy(a).to(dev)
        sink = torch.empty_like(codes)
        for radius in (1, 2, 3, 4):
            one, two, three = Smoother(radius, 1), Smoother(radius, 2), Smoother(radius, 3)
            p2, p3 = plan(radius, 2), plan(radius, 3)
            assert torch.equal(three(codes, dm), in_turn(one, one, one)(codes, dm)) and torch.equal(two(codes, dm), in_turn(one, one)(codes, dm))
            variants = {"copy_": lambda: sink.copy_(codes),
                        "passes 1": lambda: one(codes, dm),
                        f"passes 2 ({p2['launches']} launch(es), {p2['fused']} fused)": lambda: two(codes, dm),
                        "passes 2 as calls of 1 + 1": lambda: in_turn(one, one)(codes, dm),
                        f"passes 3 ({p3['launches']} launch(es), {p3['fused']} fused)": lambda: three(codes, dm),
                        f"passes 3 as calls of 2 + 1 (the first of {p2['launches']} launch(es))": lambda: in_turn(two, one)(codes, dm),
                        "passes 3 as calls of 1 + 1 + 1": lambda: in_turn(one, one, one)(codes, dm)}
            measure(f"{h}x{w} u{bits} radius {radius}", variants, rows, dict(plane=f"{h}x{w}", bits=bits, radius=radius))
    return rows


def run_kernels(dev):
    for h, w, bits in PLANES:
        a, dm = plane(np.random.default_rng(h), h, w, bits)
        codes = torch.from_numpy(a).to(dev)
        f = Smoother()
        for _ in range(200):
            f(codes, dm)
        torch.cuda.synchronize(dev)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=["calls", "rule", "kernels"])
    ap.add_argument("--json", default=None)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("No GPU found: nothing is timed without one")
    dev = torch.device("cuda:0")
    rows = []
    if a.what == "kernels":
        run_kernels(dev)
    else:
        rows = time_calls(dev) if a.what == "calls" else time_rule(dev)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "what": a.what, "rows": rows}, fh, indent=1)
    print("device", torch.cuda.get_device_name(0))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
