#!/usr/bin/env python3
"""Write tests/golden/refckpt_*.pth: checkpoints pickled by the REFERENCE's own Python (the format test.py:56-59 loads,
{"epoch", "model": <its CODONNet instance>}), so that the checkpoint tests run without the reference tree.

  python tools/make_golden_refckpt.py REFERENCE_DIR      # REFERENCE_DIR holds CODON_X4/, CODON_X8/, CODON_X16/

Each module is built and pickled in a child process whose working directory is the variant's folder, as the reference's
scripts run.  A real checkpoint holds 1.87 M fp32 weights (7.5 MB); to keep the fixtures small every parameter is first
replaced by a strided view into ONE shared storage of 32 768 seeded values (torch.save keeps views: the storage is written
once, each tensor as offset + sizes + strides).  The class names, attributes and key order in the pickle are the
reference's own.  Written per variant:

  refckpt_<mod>.pth             {"epoch": 93, "model": module}
  refckpt_<mod>_state_dict.pth  module.state_dict() of the same module (the expected values)
  refckpt_CODON_x4_lp_pools.pth {"epoch": 1, "model": module} after attention_c2.pool_types = ['avg', 'max', 'lp']
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
VARIANTS = [("CODON_X4", "CODON_x4"), ("CODON_X8", "CODON_x8"), ("CODON_X16", "CODON_x16")]

CHILD = r"""
import sys
sys.dont_write_bytecode = True
import numpy as np
import torch
import {mod} as M

N = 32768
base = torch.from_numpy((np.random.default_rng(5).standard_normal(N) * 0.05).astype(np.float32))


def view(shape, i):
    strides = [1, 5, 29, 97][:len(shape)][::-1]
    top = sum((n - 1) * s for n, s in zip(shape, strides))
    return base.as_strided(tuple(shape), tuple(strides), (i * 1543) % (N - top))


torch.manual_seed(5)
m = M.CODONNet()
for i, (name, p) in enumerate(m.named_parameters()):
    p.data = view(p.shape, i)
assert not list(m.buffers())
torch.save({{"epoch": 93, "model": m}}, {out!r} + ".pth")
torch.save(m.state_dict(), {out!r} + "_state_dict.pth")
if {lp}:
    m.attention_c2.pool_types = ["avg", "max", "lp"]
    torch.save({{"epoch": 1, "model": m}}, {out!r} + "_lp_pools.pth")
"""


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    for sub, mod in VARIANTS:
        out = os.path.join(GOLD, f"refckpt_{mod}")
        code = CHILD.format(mod=mod, out=out, lp=mod == "CODON_x4")
        subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.join(ref, sub), timeout=300,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
        print("wrote", out + "*.pth")


if __name__ == "__main__":
    main()
