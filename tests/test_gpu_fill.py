"""The pull-push hole filler on the MI355X.  The yardstick is the numpy restatement tests/fill_ref.py (pinned on the
CPU by tests/test_fill_cpu.py); the bar is EQUAL BITS throughout, no tolerance anywhere: the kernels over every shape, pattern
and format; the refusals of the C entry; and the contract of the whole path -- with the option, the depth input inference builds
from a low-resolution file is the one training builds from the same values, real pairs and synthetic degradation alike.
Shapes are the smallest at which each part can go wrong: one pixel, odd sizes, a batch, exactly one tile (the single-launch form
at its limit), one cell past the tile on both axes, four tiles across with an empty one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops, train
from codon_amd.upsample import fill_holes
from tests import fill_ref as F
from tests import train_lr_ref as T

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
P_ = C.c_void_p
quiet = lambda s: None                                               # noqa: E731


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy() if t.dtype != torch.bfloat16 else t.view(torch.int16).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


# ---- the kernels against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [f[0] for f in F.FORMATS])
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_restatement(shape, fmt):
    _, _, top, on_grid = next(f for f in F.FORMATS if f[0] == fmt)
    for pattern in F.PATTERNS:
        codes, want = F.case(shape, pattern, top), F.want(shape, pattern, top)
        if on_grid:
            src = torch.from_numpy(F.to_grid(codes, top))[:, None].cuda()
            ref = F.to_grid(want, top)[:, None]
        else:
            src, ref = _codes_dev(codes), want
        before = src.clone()
        got = fill_holes(src, None if top == 255 and not on_grid else top)
        assert got.shape == src.shape and got.dtype == src.dtype and got.data_ptr() != src.data_ptr()
        bad = np.argwhere(_bits(got) != ref.view(_bits(got).dtype))
        assert bad.size == 0, f"{shape} {fmt} {pattern}: {len(bad)} values differ, first at {bad[:3].tolist()}"
        assert torch.equal(src, before), "the argument was modified"
        if pattern in ("none", "all"):
            assert torch.equal(got, src)                             # nothing to fill / nothing to fill from: equal bits
        if pattern == "all" and on_grid:
            assert not torch.signbit(got).any()                      # a hole is +0.0


def test_plane_forms_and_dtypes():
    """(h, w) planes, uint16 tensors and a non-contiguous argument go the same way; fp32 on the 8-bit grid is the default."""
    codes, want = F.case((3, 9, 13), "levels", 65535), F.want((3, 9, 13), "levels", 65535)
    dev = _codes_dev(codes)
    one = fill_holes(dev[1])
    assert one.shape == (9, 13) and one.dtype == torch.int16 and np.array_equal(_bits(one), want[1])
    u16 = fill_holes(dev.view(torch.uint16))
    assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want)
    cut = fill_holes(dev[:, :, 2:9])
    assert np.array_equal(_bits(cut), F.fill(codes[:, :, 2:9]))
    c8, w8 = F.case((3, 9, 13), "cross", 255), F.want((3, 9, 13), "cross", 255)
    g8 = fill_holes(torch.from_numpy(F.to_grid(c8, 255))[:, None].cuda())
    assert np.array_equal(_bits(g8), F.to_grid(w8, 255)[:, None].view(np.uint32))


def test_two_streams_same_bits():
    for shape in ((2, 64, 64), (1, 70, 200)):
        codes, want = F.case(shape, "levels", 65535), F.want(shape, "levels", 65535)
        dev = _codes_dev(codes)
        torch.cuda.synchronize()
        outs = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for s in streams:
            with torch.cuda.stream(s):
                outs.append(fill_holes(dev))
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and np.array_equal(_bits(outs[0]), want)


def test_refusals_leave_out_untouched():
    lib = L.load()
    B, h, w = 1, 5, 7
    src = _codes_dev(F.case((B, h, w), "cross", 65535))
    tab = torch.zeros(65536, dtype=torch.float32, device="cuda")
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((B, h, w), -21555, dtype=torch.int16, device="cuda")
    keep_src = src.clone()

    def call(B=B, h=h, w=w, src=src.data_ptr(), fmt=L.FILL_U16, tab=tab.data_ptr(), top=65535, out=out.data_ptr(), ws=ws.data_ptr(),
             ws_bytes=None):
        need = B * lib.codon_fill_holes_workspace_bytes(h, w) if B > 0 else 0
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_fill_holes(B, h, w, p(src), fmt, p(tab), top, p(out), p(ws), ws_bytes, ops._stream(torch.device("cuda:0")))
        return st, lib.codon_last_error_string().decode()

    for kw, word in F.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("fill_holes: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="fill_holes failed with status -1: fill_holes: "):
            L.check(st, "fill_holes")
    assert "unaligned" in call(src=src.data_ptr() + 1)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and torch.equal(src, keep_src)
    assert call()[0] == 0                                            # and the good call they all differ from goes through
    assert np.array_equal(_bits(out), F.want((B, h, w), "cross", 65535))


@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 65535), (16, 10000)])
def test_one_valid_pixel_gives_a_dense_input(bits, depth_max):
    codes = _codes_dev(F.case((3, 9, 13), "one", depth_max))
    dm = depth_max if bits == 16 else None
    for dt, tdt in TORCH_DT.items():
        holey = infer.codes_to_input(codes, 4, tdt, dm)
        dense = infer.codes_to_input(fill_holes(codes, dm), 4, tdt, dm)
        assert dense.shape == (3, 1, 36, 52) and dense.dtype == tdt
        assert (holey == 0).any() and not (dense == 0).any(), dt


# ---- the end-to-end tie: inference builds training's input --------------------------------------------------------------------

def _write_holey(root, sizes, bits, depth_max, seed=0, smooth=False):
    """depth/ (codes with 6 % holes and one blob wide enough to survive the reduction) and color/: (depth dir, color dir)."""
    g = np.random.default_rng(seed)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd)
    os.makedirs(cd)
    top = 255 if bits == 8 else depth_max
    for i, (h, w) in enumerate(sizes):
        if smooth:
            yy, xx = np.mgrid[0:h, 0:w]
            v = 0.5 + 0.4 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)
            dep = np.clip(np.rint(v * top), 1, top)
            gui = np.clip(v * 255 + g.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        else:
            dep = g.integers(1, top + 1, size=(h, w))
            gui = g.integers(0, 256, size=(h, w), dtype=np.uint8)
        dep = dep.astype(np.uint8 if bits == 8 else np.uint16)
        dep[g.uniform(size=(h, w)) < 0.06] = 0
        dep[2 * h // 7:6 * h // 7, 2 * w // 7:6 * w // 7] = 0
        (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(dd, f"{i:02d}.png"), dep)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), gui)
    return dd, cd


class _Capture:
    """Stands in for the network in run_loop: keeps the depth input it was given and returns it."""

    def __init__(self):
        self.x = []

    def __call__(self, x, y):
        self.x.append(x)
        return x


@pytest.mark.parametrize("drop", [False, True], ids=["plain", "sensor_dropout"])
@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
@pytest.mark.parametrize("s, P", [(4, 32), (16, 64)])
def test_inference_input_is_trainings_input(tmp_path, s, P, bits, depth_max, drop):
    """A holey P x P image, crop = the whole image, D4 op 0.  synthesize(degrade_holes, fill_holes)'s low-resolution plane -- and
    the unfilled plane of the same call without the option -- written as PNGs of their codes and read back through
    run_loop(lr_depth=, fill_holes=True) give synthesize's x, cast to the dtype, bit for bit; the filled plane is the
    restatement's fill of the unfilled one."""
    top = 255 if bits == 8 else depth_max
    dd, cd = _write_holey(str(tmp_path), [(P, P)], bits, depth_max, seed=s + bits)
    ts = train.TrainSet(dd, cd, "cuda:0", depth_bits=bits, depth_max=depth_max if bits == 16 else 65535)
    descs = np.asarray([[int(ts.offsets[0]), P, P, 0, 0, 0]], dtype=np.int64)
    kw = dict(sensor=train.SensorModel(noise=1.0, dropout=0.3, seed=11), step=2, first_sample=1) if drop else {}
    x, _, _, lr = train.synthesize(ts, descs, s, P, degrade_holes=True, fill_holes=True, return_lr=True, **kw)
    x0, _, _, lr0 = train.synthesize(ts, descs, s, P, degrade_holes=True, return_lr=True, **kw)
    holey, filled = (F.from_grid(v.cpu().numpy()[0, 0], top) for v in (lr0, lr))
    for v, c in ((lr0, holey), (lr, filled)):                        # both planes ARE on the code grid
        assert np.array_equal(F.to_grid(c, top).view(np.uint32), v.cpu().numpy()[0, 0].view(np.uint32))
    assert (holey == 0).any() and (holey > 0).any() and not (filled == 0).any()
    assert np.array_equal(F.fill_plane(holey), filled)
    assert (x0 == 0).any() and not torch.equal(x, x0)
    dt = np.uint8 if bits == 8 else np.uint16
    dev = torch.device("cuda:0")
    for name, plane in (("holey", holey), ("filled", filled)):
        lrd = str(tmp_path / name)
        os.makedirs(lrd)
        (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(lrd, "00.png"), plane.astype(dt))
        for tdt in TORCH_DT.values():
            for pipelined in (False, True):
                m = _Capture()
                r = infer.run_loop(m, dev, tdt, None, cd, None, None, pipelined=pipelined, emit=quiet, depth_bits=bits,
                                   depth_max=depth_max if bits == 16 else 65535, lr_depth=lrd, scale=s, fill_holes=True)
                assert r["n"] == 1 and len(m.x) == 1 and m.x[0].dtype == tdt
                assert np.array_equal(_bits(m.x[0]), _bits(x.to(tdt))), (name, tdt, pipelined)
    m = _Capture()                                                    # and without the option the holes reach the network
    infer.run_loop(m, dev, torch.float32, None, cd, None, None, pipelined=False, emit=quiet, depth_bits=bits,
                   depth_max=depth_max if bits == 16 else 65535, lr_depth=str(tmp_path / "holey"), scale=s)
    assert torch.equal(m.x[0], x0)


def _d4(c, op):
    if op & 1:
        c = c.T
    if op & 2:
        c = c.flip(0)
    if op & 4:
        c = c.flip(1)
    return c


@pytest.mark.parametrize("bits, levels", [(8, 255), (16, 4096)])
@pytest.mark.parametrize("s", [4, 16])
def test_trainset_of_filled_maps(tmp_path, s, bits, levels):
    """TrainSet(lr_dir=, fill_holes=True): the pool's low-resolution planes are the restatement's fill of the files, nothing else
    in the pool moves, and synthesize's x is the D4 window of codes_to_input(fill_holes(whole file)) for all eight ops and
    windows on every border -- one launch, no host synchronisation."""
    recs, rows = T.case(s, levels)
    dd, cd, ld = T.write_set(str(tmp_path), recs, bits)
    kw = dict(depth_bits=bits, depth_max=levels if bits == 16 else 65535, lr_dir=ld, scale=s)
    ts = train.TrainSet(dd, cd, "cuda:0", fill_holes=True, **kw)
    plain = train.TrainSet(dd, cd, "cuda:0", **kw)
    assert ts.fill_holes and not plain.fill_holes and {r[5] for r in rows} == set(range(8))
    want = T.pack([(d, g, F.fill_plane(lr)) for d, g, lr in recs], bits)[0]
    assert any((lr == 0).any() for _, _, lr in recs) and not np.array_equal(want, plain.pool.cpu().numpy())
    assert np.array_equal(ts.pool.cpu().numpy(), want)
    P = T.CROPS[s]
    descs = T.descs_of(rows, ts.offsets.tolist())
    train.synthesize(ts, descs, s, P)                               # the tables go up on first use
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, y, t = train.synthesize(ts, descs, s, P, fill_holes=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    x1, y1, t1 = train.synthesize(ts, descs, s, P)                  # with this TrainSet the option changes nothing
    px, py, pt = train.synthesize(plain, descs, s, P)
    assert torch.equal(x, x1) and torch.equal(y, py) and torch.equal(t, pt) and not torch.equal(x, px)
    dm = levels if bits == 16 else None
    whole = [infer.codes_to_input(fill_holes(_codes_dev(lr), dm), s, torch.float32, dm)[0, 0] for _, _, lr in recs]
    for b, (i, H, W, y0, x0, op) in enumerate(rows):
        assert whole[i].shape == (H, W)
        assert torch.equal(x[b, 0], _d4(whole[i][y0:y0 + P, x0:x0 + P], op)), (b, i, y0, x0, op)
    with pytest.raises(ValueError, match="built with fill_holes"):
        train.synthesize(plain, descs, s, P, fill_holes=True)


def test_launch_sequences(tmp_path):
    """With the option the degradation gains exactly one codon_fill_holes between the sensor (or down) launch and the masked up
    launch; without it the calls are what they were."""
    from tests.abi_log_8bit import _acl
    dd, cd = _write_holey(str(tmp_path), [(40, 48)], 8, 255)
    ts = train.TrainSet(dd, cd, "cuda:0")
    descs = np.asarray([[int(ts.offsets[0]), 40, 48, 3, 5, k] for k in range(3)], dtype=np.int64)
    sensor = train.SensorModel(noise=1.0, dropout=0.1, seed=3)
    for kw in ({}, {"sensor": sensor}):
        train.synthesize(ts, descs, 4, 32, degrade_holes=True, fill_holes=True, **kw)      # tables and workspace
    torch.cuda.synchronize()
    real = L.load()
    names = {}
    try:
        for key, kw in (("off", {}), ("on", {"fill_holes": True}), ("sensor", {"fill_holes": True, "sensor": sensor})):
            log = _acl().install()
            torch.cuda.set_sync_debug_mode("error")
            try:
                train.synthesize(ts, descs, 4, 32, degrade_holes=True, **kw)
            finally:
                torch.cuda.set_sync_debug_mode("default")
                L._lib = real
            names[key] = [n for n, _, _ in log if n != "codon_fill_holes_workspace_bytes"]
            if key != "off":
                args = next(a for n, a, _ in log if n == "codon_fill_holes")
                assert args[:3] == [3, 8, 8] and args[4] == L.FILL_F32 and args[6] == 255
    finally:
        L._lib = real
    base = ["codon_train_crops", "codon_bicubic_downsample_masked", "codon_bicubic_upsample_masked", "codon_quantize_u8"]
    assert names["off"] == base
    assert names["on"] == base[:2] + ["codon_fill_holes"] + base[2:]
    assert names["sensor"] == base[:2] + ["codon_lr_sensor", "codon_fill_holes"] + base[2:]


# ---- the command lines ------------------------------------------------------------------------------------------------------------

def test_infer_cli_pipelined_equals_serial(tmp_path, capsys):
    from codon_amd import CODONNet
    g = np.random.default_rng(3)
    lrd, cd = str(tmp_path / "lr"), str(tmp_path / "color")
    os.makedirs(lrd)
    os.makedirs(cd)
    names = []
    for i, (h, w) in enumerate([(9, 13), (10, 16), (12, 11)]):
        lr = g.integers(1, 256, size=(h, w)).astype(np.uint8)
        lr[g.uniform(size=(h, w)) < 0.06] = 0
        lr[2:h - 2, 3:w - 3] = 0                                        # wider than the cubic's support
        io.write_gray(os.path.join(lrd, f"{i:02d}.png"), lr)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), g.integers(0, 256, size=(4 * h + 1, 4 * w + 2)).astype(np.uint8))
        names.append(f"{i:02d}.png")
    torch.manual_seed(5)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 2, "model": CODONNet()}, ck)
    for dt in ("f32", "f16"):
        outs = {}
        for mode in ("serial", "pipe", "holey"):
            od = tmp_path / f"out_{dt}_{mode}"
            capsys.readouterr()
            rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--out", str(od), "--weights", ck, "--dtype", dt]
                            + (["--serial"] if mode == "serial" else []) + ([] if mode == "holey" else ["--fill-holes"]))
            assert rc == 0
            outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in names})
        assert outs["serial"] == outs["pipe"]
        assert all(outs["holey"][1][n] != outs["pipe"][1][n] for n in names)       # the option reaches the network's input
    capsys.readouterr()


def test_fit_resumes_bit_identically_and_keeps_the_key(tmp_path):
    dd, cd = _write_holey(str(tmp_path), [(48, 40), (40, 52), (44, 44)], 8, 255, seed=2, smooth=True)
    cli = lambda *extra: ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--mask-holes", "--degrade-holes", "--crop", "32",  # noqa: E731
                          "--batch", "2", "--log-every", "1", "--seed", "5", "--dtype", "bf16", *extra]
    a, b, c, d = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth", "d.pth"))
    straight = train.main(cli("--fill-holes", "--steps", "4", "--save", a), emit=quiet)
    train.main(cli("--fill-holes", "--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(cli("--fill-holes", "--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4] and resumed["losses"] == straight["losses"][2:]
    assert all(np.isfinite(v) for _, v in straight["losses"]) and straight["losses"][0][0] == 1
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    assert ca["args"]["fill_holes"] is True and cc["args"]["fill_holes"] is True and ca["args"]["degrade_holes"] is True
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    # the key is compared on --resume, before any GPU work, either way round
    with pytest.raises(ValueError, match="fill_holes True != False"):
        train.main(cli("--steps", "4", "--resume", b), emit=quiet)
    off = train.main(cli("--steps", "2", "--save", d), emit=quiet)
    assert "fill_holes" not in torch.load(d, weights_only=False)["args"]         # a run without the option keeps its keys
    assert off["losses"] != straight["losses"][:2]
    with pytest.raises(ValueError, match="fill_holes False != True"):
        train.main(cli("--fill-holes", "--steps", "4", "--resume", d), emit=quiet)


def test_validation_fills_as_inference_does(tmp_path):
    """val["fill_holes"] reaches run_loop through validate: the means of run_loop(lr_depth=, fill_holes=True) itself."""
    from codon_amd import CODONNet
    g = np.random.default_rng(4)
    lrd, cd = str(tmp_path / "lr"), str(tmp_path / "color")
    os.makedirs(lrd)
    os.makedirs(cd)
    lr = g.integers(1, 256, size=(9, 13)).astype(np.uint8)
    lr[2:7, 3:10] = 0
    io.write_gray(os.path.join(lrd, "00.png"), lr)
    io.write_gray(os.path.join(cd, "00.png"), g.integers(0, 256, size=(36, 52)).astype(np.uint8))
    torch.manual_seed(1)
    m = CODONNet().cuda()
    dev = torch.device("cuda:0")
    val = {"lr_depth": lrd, "scale": 4, "color": cd, "label": cd, "every": 1}
    r = train.validate(m, dev, dict(val, fill_holes=True), emit=quiet)
    r0 = train.validate(m, dev, val, emit=quiet)
    m.eval()
    with torch.no_grad():
        want = infer.run_loop(m, dev, torch.float32, None, cd, cd, emit=quiet, lr_depth=lrd, scale=4, fill_holes=True)
    assert r["n"] == 1 and (r["rmse_mean"], r["ssim_mean"]) == (want["rmse_mean"], want["ssim_mean"])
    assert (r0["rmse_mean"], r0["ssim_mean"]) != (r["rmse_mean"], r["ssim_mean"])
