"""The hole-aware resampling on the MI355X.  The yardstick is the numpy restatement in
tests/resample_masked_ref.py (pinned on the CPU by tests/test_resample_masked_cpu.py); the bar is EQUAL BITS throughout: the
masked upsample, the masked downsample with its snap, the fused codes -> input kernel against both the restatement and the
three-launch composition, and the contract of the whole path -- the depth input built from a low-resolution file at
inference time is the one training builds from the same low-resolution values.  Shapes are the smallest that reach every
branch of the rule, every border, more than one block and every instantiation of the fused kernel (row lengths that are and
are not a multiple of 8 at x4)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops, train
from codon_amd.upsample import bicubic_upsample, bicubic_upsample_masked
from tests import resample_masked_ref as M
from tests import train_data16_ref as R16
from tests import train_data_ref as R

pytestmark = pytest.mark.gpu

SCALES = (4, 8, 16)
TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
P_ = C.c_void_p


def _bits_equal(got, ref, what):
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    assert g.shape == ref.shape and g.dtype == ref.dtype == np.float32, (what, g.shape, ref.shape, g.dtype)
    bad = np.argwhere(g.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {bad[:3].tolist()}"


def _cast_bits(t):
    """A device tensor of any of the three dtypes as resample_masked_ref.cast_bits states it."""
    if t.dtype == torch.bfloat16:
        return t.view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def _same(got, ref, what):
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    a, b = (v.view({2: np.uint16, 4: np.uint32}[v.dtype.itemsize]) for v in (got, ref))
    bad = np.argwhere(a != b)
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {bad[:3].tolist()}"


# ---- the masked upsample ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("shape", [(1, 5, 7), (3, 9, 13)])
def test_masked_upsample_equals_the_restatement(s, shape):
    B, h, w = shape
    for kind in M.KINDS:
        lr = M.plane(B, h, w, kind, seed=s)
        out, valid = bicubic_upsample_masked(torch.from_numpy(lr).cuda(), s)
        ro, rv = M.upsample_masked(lr, s)
        _bits_equal(out, ro, f"x{s} {shape} {kind}")
        assert valid.dtype == torch.uint8 and np.array_equal(valid.cpu().numpy(), rv.astype(np.uint8)), (s, shape, kind)
        if kind == "none":                                          # the numerator IS the existing arithmetic
            assert torch.equal(out, bicubic_upsample(torch.from_numpy(lr).cuda(), s)) and bool(valid.all())
        if kind == "all":
            assert not out.any() and not valid.any()


# ---- the masked downsample --------------------------------------------------------------------------------------------------------

def _down_masked(hr, s, levels, lut):
    lib = L.load()
    hr = torch.from_numpy(hr).cuda()
    B, _, P, _ = hr.shape
    wd = torch.from_numpy(train.down_weights(P, s)).cuda()
    tab = torch.from_numpy(np.ascontiguousarray(lut)).cuda()
    out = torch.full((B, 1, P // s, P // s), -7.0, device="cuda")
    L.check(lib.codon_bicubic_downsample_masked(B, P, s, P_(hr.data_ptr()), P_(wd.data_ptr()), P_(tab.data_ptr()), levels,
                                                P_(out.data_ptr()), ops._stream(hr.device)), "bicubic_downsample_masked")
    return out


def _down_plain(hr, s):
    lib = L.load()
    hr = torch.from_numpy(hr).cuda()
    B, _, P, _ = hr.shape
    wd = torch.from_numpy(train.down_weights(P, s)).cuda()
    out = torch.empty((B, 1, P // s, P // s), device="cuda")
    L.check(lib.codon_bicubic_downsample(B, P, s, P_(hr.data_ptr()), P_(wd.data_ptr()), P_(out.data_ptr()),
                                         ops._stream(hr.device)), "bicubic_downsample")
    return out


@pytest.mark.parametrize("s, P", [(4, 16), (4, 64), (8, 32), (16, 64)])
@pytest.mark.parametrize("levels", [255, 10000])
def test_masked_downsample_equals_the_restatement(s, P, levels):
    lv, lut = M.tables(8 if levels == 255 else 16, levels)
    assert np.array_equal(train.down_weights(P, s), R.down_weights(P, s))
    for B in (1, 9):
        for kind in M.KINDS:
            hr = M.plane(B, P, P, kind, seed=P + s, levels=levels)
            got = _down_masked(hr, s, lv, lut)
            _bits_equal(got, M.downsample_masked(hr, s, lv, lut), f"x{s} P {P} B {B} levels {levels} {kind}")
            if kind == "none":                                      # the existing kernel followed by the snap
                _bits_equal(got, M.snap(_down_plain(hr, s).cpu().numpy(), lv, lut), f"x{s} P {P} B {B} plain + snap")
                assert bool((got != 0).all())


# ---- the fused kernel ---------------------------------------------------------------------------------------------------------------

def _composition(codes_dev, s, tdt, levels, lut):
    """The three launches the fused kernel stands for: masked upsample of lut[codes], the existing quantise kernel, a cast."""
    lib = L.load()
    tab = torch.from_numpy(np.ascontiguousarray(lut)).cuda()
    idx = (codes_dev.view(torch.int16).to(torch.int64) & 0xFFFF) if codes_dev.dtype != torch.uint8 else codes_dev.to(torch.int64)
    x, _ = bicubic_upsample_masked(tab[idx][:, None].contiguous(), s)
    if levels == 255 and codes_dev.dtype == torch.uint8:
        L.check(lib.codon_quantize_u8(x.numel(), P_(x.data_ptr()), P_(tab.data_ptr()), ops._stream(x.device)), "quantize_u8")
    else:
        L.check(lib.codon_quantize_levels(x.numel(), P_(x.data_ptr()), P_(tab.data_ptr()), levels, ops._stream(x.device)),
                "quantize_levels")
    return x.to(tdt)


@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("dt", ["f32", "f16", "bf16"])
@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 65535), (16, 4096)])
def test_fused_codes_to_input(s, dt, bits, depth_max):
    lv, lut = M.tables(bits, depth_max)
    g = np.random.default_rng(7 * s + bits)
    for B, h, w in [(2, 9, 13), (1, 5, 6)]:                         # x4: row lengths 52 (no multiple of 8) and 24
        for kind in M.KINDS:
            codes = g.integers(1, lv + 1, size=(B, h, w))
            codes.reshape(-1)[:2] = [1, lv]
            for b in range(B):
                codes[b][M.holes(h, w, kind, seed=s + b)] = 0
            host = codes.astype(np.uint8) if bits == 8 else codes.astype(np.uint16).view(np.int16)
            dev = torch.from_numpy(host).cuda()
            got = infer.codes_to_input(dev, s, TORCH_DT[dt], None if bits == 8 else depth_max)
            what = f"x{s} {dt} {bits}-bit max {depth_max} {(B, h, w)} {kind}"
            assert got.shape == (B, 1, h * s, w * s) and got.dtype == TORCH_DT[dt]
            _same(_cast_bits(got), M.codes_to_input(codes, s, lv, lut, dt), what + " vs the restatement")
            _same(_cast_bits(got), _cast_bits(_composition(dev, s, TORCH_DT[dt], lv, lut)), what + " vs the composition")


# ---- training's degradation ---------------------------------------------------------------------------------------------------------

def _write_set(root, sizes, bits, depth_max, label, seed=0, smooth=False):
    """depth/ with holes (the pattern of the tests plus a large blob), color/, label/ (other holes): (dirs, [(depth, label,
    guide)])."""
    g = np.random.default_rng(seed)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "label")]
    for d in dirs:
        os.makedirs(d, exist_ok=True)
    top = 255 if bits == 8 else depth_max
    wr = io.write_gray if bits == 8 else io.write_depth16
    dt = np.uint8 if bits == 8 else np.uint16
    recs = []
    for i, (h, w) in enumerate(sizes):
        if smooth:
            yy, xx = np.mgrid[0:h, 0:w]
            v = 0.5 + 0.4 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)
            dep = np.clip(np.rint(v * top), 1, top).astype(dt)
            gui = np.clip(v * 255 + g.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        else:
            dep = g.integers(1, top + 1, size=(h, w)).astype(dt)
            gui = g.integers(0, 256, size=(h, w), dtype=np.uint8)
        lab = dep.copy()
        dep[M.holes(h, w, "pattern", seed=seed + i)] = 0
        dep[2 * h // 7:6 * h // 7, 2 * w // 7:6 * w // 7] = 0            # and one blob wide enough to survive the reduction
        lab[g.uniform(size=(h, w)) < 0.05] = 0
        wr(os.path.join(dirs[0], f"{i:02d}.png"), dep)
        io.write_gray(os.path.join(dirs[1], f"{i:02d}.png"), gui)
        if label:
            wr(os.path.join(dirs[2], f"{i:02d}.png"), lab)
        recs.append((dep, lab if label else None, gui))
    return (dirs[0], dirs[1], dirs[2] if label else None), recs


def _source(recs, ts, descs, P, lut):
    """The source crops (B,1,P,P) from the arrays themselves: lut[d4(depth[window], op)]."""
    by_off = {int(o): r for o, r in zip(ts.offsets, recs)}
    return np.stack([lut[R.d4(by_off[off][0][y0:y0 + P, x0:x0 + P], op).astype(np.int64)]
                     for off, _, _, y0, x0, op in descs.tolist()])[:, None]


@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
@pytest.mark.parametrize("label", [False, True])
def test_synthesize_degrade_holes(tmp_path, bits, depth_max, label):
    """x and the low-resolution map against the restatement, y and t against the plain path, every D4 op, windows in the
    corners, x4 / x8 / x16 -- and no host synchronisation once the tables are up."""
    lv, lut = M.tables(bits, depth_max)
    (dd, cd, ld), recs = _write_set(str(tmp_path), [(37, 53), (40, 64), (70, 81)], bits, depth_max, label, seed=bits)
    ts = train.TrainSet(dd, cd, "cuda:0", label_dir=ld, depth_bits=bits, depth_max=depth_max if bits == 16 else 65535)
    for s, P in ((4, 16), (4, 32), (8, 32), (16, 64)):
        fit = [i for i in range(len(ts)) if min(ts.sizes[i]) >= P]
        rows = []
        for b in range(9):
            i = fit[b % len(fit)]
            h, w = ts.sizes[i].tolist()
            y0, x0 = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0), ((h - P) // 2, (w - P) // 2)][b % 5]
            rows.append([int(ts.offsets[i]), h, w, y0, x0, b % 8])
        descs = np.asarray(rows, dtype=np.int64)
        train.synthesize(ts, descs, s, P, degrade_holes=True)       # the tables go up on first use
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            x, y, t, lr = train.synthesize(ts, descs, s, P, degrade_holes=True, return_lr=True)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        px, py, pt = train.synthesize(ts, descs, s, P)
        assert torch.equal(y, py) and torch.equal(t, pt) and not torch.equal(x, px)
        src = _source(recs, ts, descs, P, lut)
        if not label:
            _bits_equal(t, src, f"source x{s} P {P}")
        rx, rlr = M.degrade(src, s, lv, lut)
        _bits_equal(lr, rlr, f"lr x{s} P {P} {bits}-bit label {label}")
        _bits_equal(x, rx, f"x x{s} P {P} {bits}-bit label {label}")
        assert (rlr == 0).any() and (rx == 0).any()


# ---- the end-to-end tie: inference builds training's input ---------------------------------------------------------------------------

@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
@pytest.mark.parametrize("s, P", [(4, 32), (16, 64)])
def test_inference_input_is_trainings_input(tmp_path, bits, depth_max, s, P):
    """A holey P x P image, crop = the whole image, D4 op 0: synthesize's low-resolution plane written as a PNG of its codes
    and read back through --lr-depth's input builder gives synthesize's x, cast to the dtype, bit for bit."""
    lv, lut = M.tables(bits, depth_max)
    (dd, cd, _), recs = _write_set(str(tmp_path), [(P, P)], bits, depth_max, False, seed=s + bits)
    ts = train.TrainSet(dd, cd, "cuda:0", depth_bits=bits, depth_max=depth_max if bits == 16 else 65535)
    descs = np.asarray([[int(ts.offsets[0]), P, P, 0, 0, 0]], dtype=np.int64)
    x, _, _, lr = train.synthesize(ts, descs, s, P, degrade_holes=True, return_lr=True)
    lrh = lr.cpu().numpy()[0, 0]
    codes = np.rint(lrh.astype(np.float64) * lv).astype(np.int64)
    assert np.array_equal(np.asarray(lut)[codes].view(np.uint32), lrh.view(np.uint32))       # the plane IS on the code grid
    assert (codes == 0).any() and (codes > 0).any()
    lrd = str(tmp_path / "lr")
    os.makedirs(lrd)
    (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(lrd, "00.png"), codes.astype(np.uint8 if bits == 8 else np.uint16))
    for dt, tdt in TORCH_DT.items():
        c, y, lab, H, W = infer._load_lr(lrd, cd, None, "00.png", tdt, s, bits, depth_max if bits == 16 else 65535)[:5]
        assert (H, W) == (P, P) and lab is None and y.shape == (1, 1, P, P) and y.dtype == tdt
        got = infer.codes_to_input(c.cuda(), s, tdt, depth_max if bits == 16 else None)
        _same(_cast_bits(got), _cast_bits(x.to(tdt)), f"x{s} {bits}-bit {dt}")


# ---- the infer command line ------------------------------------------------------------------------------------------------------------

def test_infer_cli_lr_depth(tmp_path, capsys):
    from codon_amd import CODONNet
    g = np.random.default_rng(3)
    lrd, cd, ld = (str(tmp_path / n) for n in ("lr", "color", "label"))
    for d in (lrd, cd, ld):
        os.makedirs(d)
    sizes, labels = [(9, 13), (10, 16), (12, 11)], {}
    for i, (h, w) in enumerate(sizes):
        lr = g.integers(1, 256, size=(h, w)).astype(np.uint8)
        lr[M.holes(h, w, "pattern", seed=i)] = 0
        lab = g.integers(0, 256, size=(4 * h + 2, 4 * w + 3)).astype(np.uint8)      # guidance and label are cropped top-left
        io.write_gray(os.path.join(lrd, f"{i:02d}.png"), lr)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g.integers(0, 256, size=(4 * h + 1, 4 * w + 2)).astype(np.uint8))
        io.write_gray(os.path.join(ld, f"{i:02d}.png"), lab)
        labels[f"{i:02d}.png"] = lab[:4 * h, :4 * w]
    torch.manual_seed(5)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 2, "model": CODONNet()}, ck)
    for dt in ("f32", "f16"):
        outs = {}
        for mode in ("serial", "pipe"):
            od = tmp_path / f"out_{dt}_{mode}"
            capsys.readouterr()
            rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", ld, "--out", str(od), "--weights", ck,
                             "--dtype", dt] + (["--serial"] if mode == "serial" else []))
            assert rc == 0
            outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in labels})
        assert outs["serial"] == outs["pipe"]
        lines = outs["pipe"][0].splitlines()
        assert len(lines) == 1 + 3 + 2
        rms = []
        for ln, (name, lab) in zip(lines[1:4], sorted(labels.items())):
            f, rm, ss = ln.split()
            out = io.read_gray(str(tmp_path / f"out_{dt}_pipe" / name))
            assert f == name and out.shape == lab.shape
            sq, c = R16.masked_sqerr(lab, out)
            assert float(rm) == math.sqrt(sq / c) and -1.0 <= float(ss) <= 1.0
            rms.append(float(rm))
        assert float(lines[5].split()[0]) == sum(rms) / 3
    small = str(tmp_path / "small")
    os.makedirs(small)
    for i, (h, w) in enumerate(sizes):
        io.write_gray(os.path.join(small, f"{i:02d}.png"), np.zeros((4 * h - 1, 4 * w), dtype=np.uint8))
    with pytest.raises(ValueError, match=r"small.00\.png.*smaller than the 36x52"):
        infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", small, "--serial", "--weights", ck])
    with pytest.raises(ValueError, match=r"small.00\.png.*smaller than the 36x52"):
        infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", small, "--serial", "--weights", ck])
    capsys.readouterr()


# ---- training --------------------------------------------------------------------------------------------------------------------------

def test_fit_degrade_holes_resumes_bit_identically(tmp_path):
    (dd, cd, _), _ = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)], 8, 255, False, seed=2, smooth=True)
    cli = lambda *extra: ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--mask-holes", "--degrade-holes", "--crop", "32",  # noqa: E731
                          "--batch", "2", "--log-every", "1", "--seed", "5", "--dtype", "bf16", *extra]
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    quiet = lambda s: None                                               # noqa: E731
    straight = train.main(cli("--steps", "4", "--save", a), emit=quiet)
    train.main(cli("--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(cli("--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4] and resumed["losses"] == straight["losses"][2:]
    assert all(np.isfinite(v) for _, v in straight["losses"]) and straight["losses"][0][0] == 1
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"] and ca["args"]["degrade_holes"] is True
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    with pytest.raises(ValueError, match="degrade_holes True != False"):
        train.main([v for v in cli("--steps", "4", "--resume", b) if v != "--degrade-holes"], emit=quiet)


def test_validation_reads_low_resolution_maps(tmp_path):
    """--val-lr-depth reaches run_loop through validate: the same means as run_loop(lr_depth=) itself."""
    from codon_amd import CODONNet
    g = np.random.default_rng(4)
    lrd, cd = str(tmp_path / "lr"), str(tmp_path / "color")
    os.makedirs(lrd)
    os.makedirs(cd)
    lr = g.integers(1, 256, size=(9, 13)).astype(np.uint8)
    lr[M.holes(9, 13, "pattern")] = 0
    io.write_gray(os.path.join(lrd, "00.png"), lr)
    io.write_gray(os.path.join(cd, "00.png"), g.integers(0, 256, size=(36, 52)).astype(np.uint8))
    torch.manual_seed(1)
    m = CODONNet().cuda()
    dev = torch.device("cuda:0")
    r = train.validate(m, dev, {"lr_depth": lrd, "scale": 4, "color": cd, "label": cd, "every": 1}, emit=lambda s: None)
    m.eval()
    with torch.no_grad():
        want = infer.run_loop(m, dev, torch.float32, None, cd, cd, emit=lambda s: None, lr_depth=lrd, scale=4)
    assert r["n"] == 1 and (r["rmse_mean"], r["ssim_mean"]) == (want["rmse_mean"], want["ssim_mean"])
