#!/usr/bin/env python3
"""Record the checkpoint args the training command line writes: tests/golden/train_args.json.

    python tools/make_golden_train_args.py [--commit REV] [--out FILE]

For every command line of MATRIX (each after PREFIX): train.run_args(train.parse_args(argv)), the dict --resume compares and a
checkpoint's "args" start from.  No GPU is needed.  Run it in a checkout of the commit whose behaviour is to be kept (--commit
names it, for the provenance), commit the file, and tests/test_train_options_cpu.py holds every later train.py to it: the file
is never written again from the code under test."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PREFIX = "--scale 4 --train-depth d --train-color c"
MATRIX = (
    "",
    "--train-label l --mask-holes --min-valid 0.25",
    "--depth-bits 16 --depth-max 10000",
    "--degrade-holes",
    "--degrade-holes --fill-holes",
    "--train-lr-depth l --fill-holes --fill-guided --fill-sigma 6 --normalize",
    "--degrade-holes --sensor-noise 1.5 --sensor-dropout 0.05 --seed 9",
    "--lr-schedule cosine --steps 50 --warmup-steps 5 --lr-min 1e-6",
    "--lr-schedule cosine --steps 50 --lr-steps 200",
    "--clip-norm 1 --skip-nonfinite --ema 0.999",
    "--dtype f32 --crop 64 --batch 4",
    # beyond the least the matrix must hold: every option at once on either path, and the rest of the sensor model
    "--train-label l --mask-holes --depth-bits 16 --degrade-holes --fill-holes --sensor-noise 2 --sensor-noise-quad 3 "
    "--sensor-edge-dropout 0.3 --sensor-edge-threshold 12 --lr-schedule cosine --clip-norm 0.5 --ema 0.9",
    "--train-lr-depth l --normalize --depth-bits 16 --depth-max 4000 --mask-holes --min-valid 0.5",
)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--commit", default="HEAD", help="the revision of the checkout, for the provenance")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_args.json"))
    a = ap.parse_args(argv)
    from codon_amd import train
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", a.commit], check=True, capture_output=True, text=True).stdout.strip()
    doc = {"provenance": {"commit": commit, "writer": "tools/make_golden_train_args.py"}, "prefix": PREFIX,
           "runs": [{"argv": m, "args": train.run_args(train.parse_args((PREFIX + " " + m).split()))} for m in MATRIX]}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(f"{a.out}: {len(MATRIX)} command lines, {os.path.getsize(a.out)} bytes")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
