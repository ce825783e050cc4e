"""The ordered ABI call log (tools/abi_call_log.py) of the 8-bit defaults -- TEST INFRASTRUCTURE: two training steps of
`codon_amd.train` with the CLI's defaults (x4, crop 128, batch 16, bf16) and one image through `codon_amd.infer`'s serial
loop (f16, with a label), on a small synthetic 8-bit set.  Nothing here names an option that postdates the 8-bit path, so
the same function runs on any commit; tests/golden/abi_log_8bit.json is what it returned on the commit before 16-bit depth
maps were added."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _acl():
    spec = importlib.util.spec_from_file_location("abi_call_log", os.path.join(ROOT, "tools", "abi_call_log.py"))
    acl = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(acl)
    return acl


def write_set(root):
    from codon_amd import io
    rng = np.random.default_rng(11)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd)
    os.makedirs(cd)
    for i, (h, w) in enumerate([(130, 141), (150, 128)]):
        yy, xx = np.mgrid[0:h, 0:w]
        d = (127.5 + 100 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)).astype(np.uint8)
        g = np.clip(d.astype(int) + rng.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g)
    return dd, cd


def record(root):
    """{"train": [[name, args], ...], "infer": [...]} -- return values left out (they are all 0 or sizes)."""
    from codon_amd import CODONNet, infer, train
    from codon_amd import _lib as L
    acl = _acl()
    dd, cd = write_set(root)
    real = L.load()
    ts = train.TrainSet(dd, cd, "cuda:0", crop=128)
    quiet = lambda s: None                                               # noqa: E731
    train.fit(CODONNet().cuda(), ts, 1, scale=4, emit=quiet)             # once-per-process work stays out of the log
    logs = {}
    try:
        torch.manual_seed(0)
        m = CODONNet().cuda()
        log = acl.install()
        train.fit(m, ts, 2, scale=4, seed=3, log_every=1, emit=quiet)
        logs["train"] = [[n, a] for n, a, _ in log]
        L._lib = real
        dev = torch.device("cuda:0")
        m = CODONNet().to(dev).to(torch.float16).eval()
        infer.run_loop(m, dev, torch.float16, dd, cd, dd, None, pipelined=False, emit=quiet, files=["00.png"])   # warm
        log = acl.install()
        infer.run_loop(m, dev, torch.float16, dd, cd, dd, None, pipelined=False, emit=quiet, files=["00.png"])
        logs["infer"] = [[n, a] for n, a, _ in log]
    finally:
        L._lib = real
    return logs
