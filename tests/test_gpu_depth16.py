"""16-bit depth maps end to end on the MI355X.  The yardstick is the numpy restatement in
tests/train_data16_ref.py (pinned on the CPU by tests/test_depth16_cpu.py): crops, the whole synthesis, the quantisation
onto the code grid, the post-processing and the squared error are held to EQUAL BITS / exact integers; the tie to the 8-bit
path is lut16(65535)[257 k] == u8_lut()[k].  The step-1 loss bar, 2e-6, is the one tests/test_gpu_masked_loss.py holds the
masked loss to.  Shapes are the smallest that reach every branch: odd H*W (padding), windows on every border, batch 1 / 9 /
64, crop 16 / 32 / 64."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch

from codon_amd import io, train
from tests import train_data16_ref as R16
from tests import train_data_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(37, 53), (40, 64), (70, 81)]


def _bits_equal(got, ref, what):
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    assert g.shape == ref.shape and g.dtype == ref.dtype == np.float32, (what, g.shape, ref.shape)
    bad = np.argwhere(g.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {bad[:3].tolist()}"


def _descs(ts, P, B):
    """B rows over the images that hold a P x P window: every D4 code, the window in the four corners and in the middle of
    the four borders, in turn."""
    rows = []
    fit = [i for i in range(len(ts)) if min(ts.sizes[i]) >= P]
    for b in range(B):
        i = fit[b % len(fit)]
        off, (h, w) = int(ts.offsets[i]), ts.sizes[i].tolist()
        ym, xm = (h - P) // 2, (w - P) // 2
        y0, x0 = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0), (0, xm), (h - P, xm), (ym, 0), (ym, w - P)][(b // 8 + b) % 8]
        rows.append([off, h, w, y0, x0, b % 8])
    return np.asarray(rows, dtype=np.int64)


def _crops16(ts, descs, P):
    """codon_train_crops_u16 alone: (source, guide, target or None)."""
    from codon_amd import _lib as L
    from codon_amd import ops
    lib = L.load()
    dev = ts.pool.device
    d = L.CropDesc()
    d.n, d.crop = len(descs), P
    for b, (off, h, w, y0, x0, op) in enumerate(descs.tolist()):
        s = d.s[b]
        s.offset, s.height, s.width, s.y0, s.x0, s.op = off, h, w, y0, x0, op
    t16 = torch.from_numpy(train.lut16(ts.depth_max)).to(dev)
    t8 = torch.from_numpy(train.u8_lut()).to(dev)
    src, gui, tgt = (torch.full((len(descs), 1, P, P), -7.0, device=dev) for _ in range(3))
    P_ = C.c_void_p
    with ops._on(dev):
        L.check(lib.codon_train_crops_u16(C.byref(d), P_(ts.pool.data_ptr()), ts.pool.numel(), P_(t16.data_ptr()), P_(t8.data_ptr()),
                                          P_(src.data_ptr()), P_(gui.data_ptr()), P_(tgt.data_ptr()) if ts.has_label else None,
                                          ops._stream(dev)), "train_crops_u16")
    return src, gui, (tgt if ts.has_label else None)


# ---- crops -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("depth_max", [65535, 10000, 4096])
@pytest.mark.parametrize("label", [False, True])
def test_crops_equal_bits(tmp_path, label, depth_max):
    dd, cd, ld, recs = R16.write_set(str(tmp_path), SIZES, label=label, seed=depth_max, depth_max=depth_max)
    ts = train.TrainSet(dd, cd, "cuda:0", label_dir=ld, depth_bits=16, depth_max=depth_max)
    pool = ts.pool.cpu().numpy()
    assert np.array_equal(pool, R16.pack(recs)[0]) and all(o % 2 == 0 for o in ts.offsets.tolist())
    for P in (16, 32, 64):                                         # 64 fits the 70x81 image alone
        for B in (1, 9, 64):
            descs = _descs(ts, P, B)
            src, gui, tgt = _crops16(ts, descs, P)
            rs, ry, rt = R16.crops(pool, descs, P, depth_max, label)
            _bits_equal(src, rs, f"source P{P} B{B}")
            _bits_equal(gui, ry, f"guide P{P} B{B}")
            if label:
                _bits_equal(tgt, rt, f"target P{P} B{B}")
                assert not np.array_equal(rs, rt)
    vals = src.cpu().numpy()                                         # P = 64, B = 64: codes 0, 1 and depth_max are in the image
    tab = R16.lut16(depth_max)
    if label:
        assert (tgt == 0).any()
    for code in (0, 1, depth_max):
        full = torch.from_numpy(np.asarray([[int(ts.offsets[0]), 37, 53, 0, 0, 0]], dtype=np.int64))
        s0 = _crops16(ts, full.numpy(), 16)[0].cpu().numpy()
        assert (s0.view(np.uint32) == tab[code:code + 1].view(np.uint32)).any(), code
    assert vals.min() >= 0.0 and vals.max() <= 1.0


def _write8(root, sizes, seed=0):
    g = np.random.default_rng(seed)
    dirs = [os.path.join(root, n) for n in ("depth8", "color8", "label8")]
    recs = []
    for d in dirs:
        os.makedirs(d)
    for i, (h, w) in enumerate(sizes):
        dep = g.integers(0, 256, (h, w), dtype=np.uint8)
        gui = g.integers(0, 256, (h, w), dtype=np.uint8)
        lab = g.integers(0, 256, (h, w), dtype=np.uint8)
        lab[g.uniform(size=(h, w)) < 0.1] = 0
        for d, a in zip(dirs, (dep, gui, lab)):
            io.write_gray(os.path.join(d, f"{i:02d}.png"), a)
        recs.append((dep, lab, gui))
    return dirs, recs


@pytest.mark.parametrize("label", [False, True])
def test_tie_to_the_8bit_path(tmp_path, label):
    """257 x an 8-bit set at depth_max 65535: lut16[257 k] is u8_lut[k], so t and y are the 8-bit path's bits (x is not held:
    its grid is finer)."""
    (d8, c8, l8), recs = _write8(str(tmp_path), SIZES, seed=4)
    d16, l16 = str(tmp_path / "depth16"), str(tmp_path / "label16")
    os.makedirs(d16)
    os.makedirs(l16)
    for i, (dep, lab, _) in enumerate(recs):
        io.write_depth16(os.path.join(d16, f"{i:02d}.png"), dep.astype(np.uint16) * 257)
        io.write_depth16(os.path.join(l16, f"{i:02d}.png"), lab.astype(np.uint16) * 257)
    ts8 = train.TrainSet(d8, c8, "cuda:0", label_dir=l8 if label else None)
    ts16 = train.TrainSet(d16, c8, "cuda:0", label_dir=l16 if label else None, depth_bits=16)
    for P, s in ((16, 4), (32, 8), (64, 16)):
        a, b = _descs(ts8, P, 9), _descs(ts16, P, 9)
        assert np.array_equal(a[:, 1:], b[:, 1:])
        x8, y8, t8 = train.synthesize(ts8, a, s, P)
        x16, y16, t16 = train.synthesize(ts16, b, s, P)
        assert torch.equal(t8.view(torch.int32), t16.view(torch.int32)) and torch.equal(y8.view(torch.int32), y16.view(torch.int32))
        assert float((x8 - x16).abs().max()) <= 0.5 / 255 + 1e-6        # the same degradation, on a finer grid


# ---- the whole synthesis -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("scale,P", [(4, 16), (8, 32), (16, 64)])
def test_synthesize_equal_bits(tmp_path, scale, P):
    for label, depth_max in ((True, 10000), (False, 65535)):
        root = str(tmp_path / f"s{int(label)}")
        dd, cd, ld, _ = R16.write_set(root, SIZES, label=label, seed=scale, depth_max=depth_max)
        ts = train.TrainSet(dd, cd, "cuda:0", crop=P if P < 64 else None, label_dir=ld, depth_bits=16, depth_max=depth_max)
        descs = _descs(ts, P, 9)
        train.synthesize(ts, descs, scale, P)                         # the tables go up on first use, as the 8-bit ones do
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")                       # after that: no synchronisation inside synthesize
        try:
            x, y, t = train.synthesize(ts, descs, scale, P)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        rx, ry, rt = R16.synthesize(ts.pool.cpu().numpy(), descs, scale, P, depth_max, label)
        for got, ref, n in ((t, rt, "t"), (y, ry, "y"), (x, rx, "x")):
            _bits_equal(got, ref, f"{n} x{scale} label {label}")
        assert not np.array_equal(rx, rt)
        grid = set(np.unique(R16.lut16(depth_max)[:depth_max + 1]).tolist())
        assert set(np.unique(x.cpu().numpy()).tolist()) <= grid       # x lies on the data set's own code grid


# ---- quantise, post-process, squared error -------------------------------------------------------------------------------------

def _special(depth_max):
    g = np.random.default_rng(depth_max)
    k = np.arange(depth_max, dtype=np.float64)
    ties = ((k + 0.5) / depth_max).astype(np.float32)
    odd = np.array([-1.0, -1e-30, -0.0, 0.0, 1e-45, 1e-39, 1.1754944e-38, 1.0, 1.0000001, 2.0, 1e30, np.inf, -np.inf],
                   dtype=np.float32)
    return np.concatenate([ties, odd, g.uniform(-0.2, 1.2, 37 * 53 - 13).astype(np.float32)])


@pytest.mark.parametrize("depth_max", [4096, 10000, 65535])
def test_quantize_levels_equal_bits(depth_max):
    from codon_amd import _lib as L
    from codon_amd import ops
    lib = L.load()
    x = _special(depth_max)
    if depth_max == 4096:
        assert np.array_equal(x[:4096].astype(np.float64) * 4096, np.arange(4096) + 0.5)      # exact ties
    xd = torch.from_numpy(np.concatenate([x, np.array([np.nan, -np.nan], dtype=np.float32)])).cuda()
    tab = torch.from_numpy(train.lut16(depth_max)).cuda()
    with ops._on(xd.device):
        L.check(lib.codon_quantize_levels(xd.numel(), C.c_void_p(xd.data_ptr()), C.c_void_p(tab.data_ptr()), depth_max,
                                          ops._stream(xd.device)), "quantize_levels")
    got = xd.cpu().numpy()
    _bits_equal(got[:-2], R16.quantize(x, depth_max), f"quantize_levels {depth_max}")
    # the stated rule, not numpy's: NaN -> lut16[0], which is +0.0
    assert got[-2:].view(np.uint32).tolist() == [0, 0] and train.lut16(depth_max)[0].view(np.uint32) == 0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16])
def test_postprocess_u16_equals_the_restatement(dtype):
    from codon_amd import metrics
    for depth_max in (4096, 10000, 65535):
        v = _special(depth_max)
        # the first 512 ties in a row ((2k + 1) / 8192 is exact in fp16 for k < 1024 and in bf16 for k < 128), 512 spread over
        # the range, the special values, random ones
        v = np.concatenate([v[:512], v[512:depth_max:max(1, depth_max // 512)][:512], v[depth_max:]])[:37 * 53 - 1]
        x = torch.from_numpy(np.concatenate([v, np.array([np.nan], dtype=np.float32)])).to(dtype).reshape(37, 53)
        if dtype == torch.bfloat16:
            host = x.view(torch.int16).numpy().view(np.uint16)        # bf16 bit patterns
            f32 = (host.astype(np.uint32) << 16).view(np.float32)
        else:
            host = x.numpy()
            f32 = host.astype(np.float32)
        want = R16.postprocess_u16(host, depth_max)
        got = metrics.postprocess_u16(x.cuda(), depth_max)
        assert got.dtype == torch.uint16 and got.shape == (37, 53)
        got = got.cpu().numpy()
        assert np.array_equal(got, want), np.argwhere(got != want)[:3]
        assert got[-1, -1] == 0 and want.max() == depth_max and want.min() == 0          # NaN -> 0; > 1 -> depth_max
        prod = np.clip(f32[np.isfinite(f32)].astype(np.float64), 0, 1) * depth_max
        if depth_max == 4096:
            assert (np.abs(prod - np.floor(prod)) == 0.5).sum() >= 100                    # ties survive the cast to every dtype


def test_masked_rmse_u16_is_exact():
    from codon_amd import metrics
    g = np.random.default_rng(1)
    cases = []
    lab = g.integers(0, 65536, (37, 53)).astype(np.uint16)
    lab[g.uniform(size=lab.shape) < 0.2] = 0
    cases.append((lab, g.integers(0, 65536, (37, 53)).astype(np.uint16)))
    ext = np.full((40, 64), 65535, dtype=np.uint16)                     # extreme differences on every valid pixel
    ext[::3] = 0
    out = np.zeros((40, 64), dtype=np.uint16)
    out[::3] = 65535                                                     # ... and on the holes, where they must not count
    cases.append((ext, out))
    one = np.zeros((37, 53), dtype=np.uint16)
    one[17, 29] = 3
    cases.append((one, np.full((37, 53), 65535, dtype=np.uint16)))
    cases.append((np.pad(lab, ((0, 2), (0, 3))), cases[0][1]))          # a larger label is cropped to the output
    for lab, out in cases:
        s, c = R16.masked_sqerr(lab, out)
        ld, od = torch.from_numpy(lab.view(np.int16)).cuda(), torch.from_numpy(out).cuda()
        acc = metrics.masked_sqerr_u16_dev(ld, od)
        assert acc.dtype == torch.int64 and acc.cpu().tolist() == [s, c]
        assert metrics.masked_rmse_u16(ld.view(torch.uint16), od.view(torch.int16)) == math.sqrt(s / c)
    assert R16.masked_sqerr(*cases[1]) == (65535 ** 2 * (40 * 64 - 14 * 64), 40 * 64 - 14 * 64)
    assert R16.masked_sqerr(*cases[2]) == ((65535 - 3) ** 2, 1)


# ---- the infer command line ------------------------------------------------------------------------------------------------------

def test_infer_cli_16bit(tmp_path, capsys):
    from PIL import Image
    from codon_amd import CODONNet, infer
    depth_max, unit = 10000, 0.1
    dd, cd, ld, recs = R16.write_set(str(tmp_path), [(37, 53), (40, 64), (37, 53), (40, 64)], seed=8, depth_max=depth_max)
    full = recs[1][1].copy()
    full[full == 0] = 1
    io.write_depth16(os.path.join(ld, "01.png"), full)                  # one label without holes, three with
    labels = {f"{i:02d}.png": (full if i == 1 else r[1]) for i, r in enumerate(recs)}
    torch.manual_seed(5)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 2, "model": CODONNet()}, ck)
    for dt in ("f32", "f16"):
        outs = {}
        for mode in ("serial", "pipe"):
            od = tmp_path / f"out_{dt}_{mode}"
            capsys.readouterr()
            rc = infer.main(["--scale", "4", "--input-depth", dd, "--input-color", cd, "--label", ld, "--out", str(od), "--weights", ck,
                             "--dtype", dt, "--depth-bits", "16", "--depth-max", str(depth_max), "--depth-unit", str(unit)] +
                            (["--serial"] if mode == "serial" else []))
            assert rc == 0
            outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in labels})
        assert outs["serial"] == outs["pipe"]
        lines = outs["pipe"][0].splitlines()
        assert len(lines) == 1 + 4 + 2
        rms = []
        for ln, (name, lab) in zip(lines[1:5], sorted(labels.items())):
            f, rm, ss = ln.split()
            p = str(tmp_path / f"out_{dt}_pipe" / name)
            assert f == name and Image.open(p).mode in io.DEPTH16_MODES
            out = io.read_depth(p)
            assert out.dtype == np.uint16 and out.shape == lab.shape and out.max() <= depth_max
            s, c = R16.masked_sqerr(lab, out)
            assert float(rm) == math.sqrt(s / c) * unit and -1.0 <= float(ss) <= 1.0
            rms.append(float(rm))
        assert float(lines[6].split()[0]) == sum(rms) / 4
        assert len({bytes(v) for v in outs["pipe"][1].values()}) == 4
    with pytest.raises(ValueError, match=r"00\.png.*--depth-bits 16"):                    # the same files as 8-bit: refused
        infer.main(["--input-depth", dd, "--input-color", cd, "--serial", "--weights", ck])
    with pytest.raises(ValueError, match=r"depth.0[0-3]\.png.*--depth-bits 16"):                # whichever reader got there first
        infer.main(["--input-depth", dd, "--input-color", cd, "--weights", ck])
    capsys.readouterr()


# ---- training ----------------------------------------------------------------------------------------------------------------------

def _smooth16(root, sizes, depth_max, seed=0):
    """Something to learn: smooth 16-bit depth, a noisy 8-bit guidance, labels = depth with holes."""
    g = np.random.default_rng(seed)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "label")]
    for d in dirs:
        os.makedirs(d)
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        v = 0.5 + 0.4 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)
        dep = np.clip(np.rint(v * depth_max), 1, depth_max).astype(np.uint16)
        lab = dep.copy()
        lab[g.uniform(size=(h, w)) < 0.05] = 0
        lab[3:9, 5:14] = 0
        gui = np.clip(v * 255 + g.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        io.write_depth16(os.path.join(dirs[0], f"{i:02d}.png"), dep)
        io.write_gray(os.path.join(dirs[1], f"{i:02d}.png"), gui)
        io.write_depth16(os.path.join(dirs[2], f"{i:02d}.png"), lab)
    return dirs


def _cli(dd, cd, ld, *extra):
    return ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--train-label", ld, "--mask-holes", "--min-valid", "0.5",
            "--crop", "32", "--batch", "2", "--log-every", "1", "--seed", "5", "--depth-bits", "16", "--depth-max", "10000", *extra]


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_fit16_resumes_bit_identically(tmp_path, dtype):
    dd, cd, ld = _smooth16(str(tmp_path), [(48, 40), (40, 52), (44, 44)], 10000)
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    quiet = lambda s: None                                               # noqa: E731
    straight = train.main(_cli(dd, cd, ld, "--dtype", dtype, "--steps", "4", "--save", a), emit=quiet)
    train.main(_cli(dd, cd, ld, "--dtype", dtype, "--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(_cli(dd, cd, ld, "--dtype", dtype, "--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4] and resumed["losses"] == straight["losses"][2:]
    assert all(np.isfinite(v) for _, v in straight["losses"])
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    assert ca["optimizer"]["t"] == cc["optimizer"]["t"] == 4
    for p, q in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q)
    assert (ca["args"]["depth_bits"], ca["args"]["depth_max"]) == (16, 10000)
    with pytest.raises(ValueError, match="depth_max 10000 != 4096"):      # another scale of the codes: another trajectory
        other = ["4096" if v == "10000" else v for v in _cli(dd, cd, ld, "--dtype", dtype, "--steps", "4", "--resume", b)]
        train.main(other, emit=quiet)


def test_8bit_checkpoint_keeps_its_keys_and_resumes(tmp_path):
    from tests.test_depth16_cpu import PARENT_ARG_KEYS
    (d8, c8, _), _ = _write8(str(tmp_path), [(40, 48), (36, 50)])
    base = ["--scale", "4", "--train-depth", d8, "--train-color", c8, "--crop", "32", "--batch", "2", "--log-every", "1"]
    p = str(tmp_path / "k.pth")
    quiet = lambda s: None                                               # noqa: E731
    train.main(base + ["--steps", "1", "--save", p], emit=quiet)
    ck = torch.load(p, weights_only=False)
    assert set(ck["args"]) == PARENT_ARG_KEYS                              # no depth_bits, no depth_max: the keys it always had
    r = train.main(base + ["--steps", "2", "--resume", p], emit=quiet)     # ... and it resumes under the defaults
    assert [s for s, _ in r["losses"]] == [2]


def test_fit16_step_one_loss(tmp_path):
    from codon_amd import CODONNet
    from tests import masked_loss_ref as M
    dd, cd, ld = _smooth16(str(tmp_path), [(48, 40), (40, 52), (44, 44)], 10000)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32, label_dir=ld, depth_bits=16, depth_max=10000)
    torch.manual_seed(0)
    m = CODONNet().cuda()
    seen = []
    h = m.register_forward_hook(lambda mod, inp, out: seen.append(out.detach().float().clone()))
    r = train.fit(m, ts, 1, scale=4, crop=32, batch=4, dtype="f32", seed=9, log_every=1, emit=lambda s: None, mask_holes=True,
                  min_valid=0.5)
    h.remove()
    descs = train.draw(np.random.default_rng(9), ts, 4, 32, min_valid=0.5)      # the rows fit drew
    _, _, t = train.synthesize(ts, descs, 4, 32)
    assert len(seen) == 1 and (t == 0).any()
    ref = float(M.masked_loss(seen[0].double().cpu(), t.double().cpu()))
    got = r["losses"][0][1]
    print(f"16-bit step-1 loss {got:.8f}, float64 restatement on the step's own output {ref:.8f}, |d| {abs(got - ref):.3e} (bar 2e-6)")
    assert abs(got - ref) < 2e-6


# ---- the 8-bit defaults issue the calls they always issued ---------------------------------------------------------------------------

def test_8bit_defaults_issue_the_recorded_calls(tmp_path):
    """The ordered ABI call log of two default training steps and of one infer image, against the log recorded with
    tests/abi_log_8bit.py on the commit before this path existed (tests/golden/abi_log_8bit.json)."""
    from tests import abi_log_8bit as A
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_log_8bit.json")))
    got = json.loads(json.dumps(A.record(str(tmp_path))))
    acl = A._acl()
    for leg in ("train", "infer"):
        assert acl.diff([c + [0] for c in want[leg]], [c + [0] for c in got[leg]]) is None, leg
        assert not any(n.endswith(("_u16", "_u16_dt", "quantize_levels")) for n, _ in got[leg])
    assert len(got["train"]) > 200 and len(got["infer"]) > 20
