"""The ordered ABI call log (tools/abi_call_log.py) of the low-resolution depth preparation -- TEST INFRASTRUCTURE: hole filling,
guided filling and range normalisation through every public path that threads them -- infer.run_loop in
both loops, train.TrainSet, train.synthesize and train.validate -- on a tiny synthetic set, 8-bit and 16-bit, with a stand-in
network that returns its depth input so that no convolution is in the log.  Only keyword arguments and `val` keys are used, so the
same function runs on any commit that has the options; tests/golden/abi_log_prep.json is what it returned on commit
a01dac3 ("Add guidance-aware hole filling: joint pull-push, --fill-guided"), the parent of the change that gave the
preparation one record."""
import hashlib
import os

import numpy as np
import torch

from tests.abi_log_8bit import _acl

SIGMA = 6.0                 # not the default: a sigma lost on the way shows in the hashes
COMBOS = {"off": {},
          "fill": {"fill_holes": True},
          "fill_guided": {"fill_holes": True, "fill_guided": True, "fill_sigma": SIGMA},
          "normalize": {"normalize": True},
          "fill_normalize": {"fill_holes": True, "normalize": True},
          "fill_guided_normalize": {"fill_holes": True, "fill_guided": True, "fill_sigma": SIGMA, "normalize": True}}
FORMATS = {"u8": (8, 255), "u16": (16, 1000)}
quiet = lambda s: None                                               # noqa: E731


class Stub:
    """Stands in for the network: keeps the depth input it was given and returns it."""

    def __init__(self):
        self.x = []

    def __call__(self, x, y):
        self.x.append(x)
        return x

    def eval(self):
        return self

    def train(self):
        return self


def write_set(root, bits, top, n=2):
    """n (two) pairs of 40 x 48 with 10 x 12 low-resolution maps that carry holes, and the depth maps once more with holes of their
    own: [depth dir, color dir, lr dir, holey depth dir]"""
    from codon_amd import io
    g = np.random.default_rng(1)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "lr", "holey")]
    for d in dirs:
        os.makedirs(d)
    write = io.write_gray if bits == 8 else io.write_depth16
    dt = np.uint8 if bits == 8 else np.uint16
    for i in range(n):
        lr = g.integers(1, top + 1, size=(10, 12))
        lr[g.random((10, 12)) < 0.25] = 0
        lr[3 + i % 2:6, 2:5 + i % 2] = 0                              # and a hole wider than one pixel
        write(os.path.join(dirs[0], f"{i:02d}.png"), g.integers(1, top + 1, size=(40, 48)).astype(dt))
        io.write_gray(os.path.join(dirs[1], f"{i:02d}.png"), g.integers(0, 256, size=(40, 48)).astype(np.uint8))
        write(os.path.join(dirs[2], f"{i:02d}.png"), lr.astype(dt))
        hr = g.integers(1, top + 1, size=(40, 48))
        hr[g.random((40, 48)) < 0.25] = 0
        write(os.path.join(dirs[3], f"{i:02d}.png"), hr.astype(dt))
    return dirs


def _sha(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


WS_BYTES = {"codon_fill_holes": 9, "codon_fill_holes_guided": 13}    # where an entry takes the capacity of its workspace


def stable(name, args):
    """[name, args] with the workspace's capacity as "cap": the per-stream workspace grows and is kept (guards.PerStream), so
    that number is the largest plane the PROCESS has filled on the stream, not a property of the call."""
    i = WS_BYTES.get(name)
    return [name, args if i is None else args[:i] + ["cap"] + args[i + 1:]]


def _logged(fn):
    """(fn's result, its calls as [name, args] without the workspace queries)"""
    from codon_amd import _lib as L
    real = L.load()
    log = _acl().install()
    try:
        r = fn()
    finally:
        L._lib = real
    return r, [stable(n, a) for n, a, _ in log if not n.endswith("_workspace_bytes")]


def _per_stream(log):
    return {s: [c[:2] for c in calls] for s, calls in _acl().per_stream([[n, a, 0] for n, a in log]).items()}


def _scenarios(dirs, bits, top, opts, logged):
    """One combination through the five paths; `logged` is _logged, or a stand-in that records nothing (the warm-up)."""
    from codon_amd import infer, train
    dd, cd, ld = dirs[:3]
    dev = torch.device("cuda:0")
    deep = {"depth_bits": 16, "depth_max": top} if bits == 16 else {}
    out = {}
    for key, pipelined in (("serial", False), ("pipelined", True)):
        m = Stub()
        _, log = logged(lambda: infer.run_loop(m, dev, torch.float32, None, cd, None, None, pipelined=pipelined, emit=quiet,
                                               lr_depth=ld, scale=4, **deep, **opts))
        out[key] = _per_stream(log) if pipelined else log
        out[key + "_input_sha256"] = _sha(m.x)
    ts, out["trainset"] = logged(lambda: train.TrainSet(dd, cd, dev, crop=32, lr_dir=ld, scale=4, **deep, **opts))
    out["pool_sha256"] = _sha([ts.pool])
    descs = np.asarray([[int(ts.offsets[i]), 40, 48, 3 + i, 5, 2 + 3 * i] for i in range(2)], dtype=np.int64)
    kw = {"fill_holes": True} if opts.get("fill_holes") else {}      # as fit calls it
    _, out["synthesize"] = logged(lambda: train.synthesize(ts, descs, 4, 32, **kw))
    val = {"lr_depth": ld, "scale": 4, "color": cd, "label": dd, "every": 1, **deep, **opts}
    _, out["validate"] = logged(lambda: train.validate(Stub(), dev, val, emit=quiet))
    return out


def _degraded(dirs, bits, top, logged):
    """synthesize(degrade_holes=True, fill_holes=True) on a set without low-resolution maps"""
    from codon_amd import train
    deep = {"depth_bits": 16, "depth_max": top} if bits == 16 else {}
    ts = train.TrainSet(dirs[3], dirs[1], "cuda:0", **deep)          # depth maps that carry holes themselves
    descs = np.asarray([[int(ts.offsets[i]), 40, 48, 3 + i, 5, 2 + 3 * i] for i in range(2)], dtype=np.int64)
    return logged(lambda: train.synthesize(ts, descs, 4, 32, degrade_holes=True, fill_holes=True))[1]


def record(root):
    """{"u8" | "u16": {combination: {"serial", "pipelined" (per stream), "trainset", "synthesize", "validate": [[name, args],
    ...], "serial_input_sha256", "pipelined_input_sha256", "pool_sha256"}, "degrade_fill": [...]}}"""
    unlogged = lambda fn: (fn(), [])                                  # noqa: E731
    logs = {}
    for fmt, (bits, top) in FORMATS.items():
        dirs = write_set(os.path.join(root, fmt), bits, top)
        for name in ("fill_normalize", "fill_guided_normalize"):     # once-per-process work stays out of the log
            _scenarios(dirs, bits, top, COMBOS[name], unlogged)
        _degraded(dirs, bits, top, unlogged)
        torch.cuda.synchronize()
        logs[fmt] = {name: _scenarios(dirs, bits, top, opts, _logged) for name, opts in COMBOS.items()}
        logs[fmt]["degrade_fill"] = _degraded(dirs, bits, top, _logged)
    return logs
