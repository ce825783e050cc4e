"""The guidance-aware pull-push hole filler on the MI355X.  The yardstick is the numpy restatement
tests/guided_fill_ref.py (pinned on the CPU by tests/test_guided_fill_cpu.py); the bar is EQUAL BITS throughout, no tolerance
anywhere: the kernels over every shape, pattern, kind of guidance, table and format; the equivalence with the plain filler under a
constant table; the refusals of the C entry; and the contract of the whole path -- with the option, the depth input inference
builds from a low-resolution file and its guidance is the one training builds from the same record.
Shapes are the plain filler's, the smallest at which each part can go wrong: one pixel, odd sizes with a guide that is the corner
of a larger image, a batch with an image stride, exactly one tile (the single-launch form at its limit), one cell past the tile on
both axes (at x16: a 1040 x 1072 guide), four tiles across with an empty one."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops, train
from codon_amd.upsample import fill_holes, fill_holes_guided, range_table
from tests import fill_ref as F
from tests import guided_fill_ref as R
from tests import train_lr_ref as T

pytestmark = pytest.mark.gpu

P_ = C.c_void_p
quiet = lambda s: None                                               # noqa: E731
FORMATS = [f for f in F.FORMATS if not f[3]]                         # u8, u16 at 65535, u16 at 10000
TABLES = (10.0, 3.0, "c37")


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy() if t.dtype != torch.bfloat16 else t.view(torch.int16).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _table_dev(table):
    return torch.from_numpy(R.table_of(table).view(np.int16).copy()).cuda()


def _guide_dev(shape, s, kind):
    """The guidance of a case on the device, held the way its row of the table of shapes says: 1 x 5 x 7 as the corner of a
    23 x 40 image (row stride > width), 3 x 9 x 13 inside taller and wider images (an image stride), else exactly sized."""
    g = R.guide_case(shape, s, kind)
    B, H, W = g.shape
    if shape == (1, 5, 7):
        big = np.full((1, 23, 40), 201, dtype=np.uint8)
    elif shape == (3, 9, 13):
        big = np.full((3, H + 5, W + 8), 201, dtype=np.uint8)
    else:
        return torch.from_numpy(g.copy()).cuda()
    big[:, :H, :W] = g
    return torch.from_numpy(big).cuda()


# ---- the kernels against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [f[0] for f in FORMATS])
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_restatement(shape, fmt):
    """Every pattern with every kind of guidance at sigma 10, and every pattern with every table under random guidance."""
    top = next(f for f in FORMATS if f[0] == fmt)[2]
    s = R.SHAPE_SCALE[shape]
    guides = {kind: _guide_dev(shape, s, kind) for kind in R.GUIDES}
    tables = {t: _table_dev(t) for t in TABLES}
    for pattern in F.PATTERNS:
        src = _codes_dev(F.case(shape, pattern, top))
        before = src.clone()
        for kind, table in [(k, 10.0) for k in R.GUIDES] + [("random", t) for t in TABLES[1:]]:
            want = R.want(shape, pattern, top, s, kind, table)
            gd = guides[kind]
            keep = gd.clone()
            got = fill_holes_guided(src, gd, s, depth_max=None if top == 255 else top, _table=tables[table])
            assert got.shape == src.shape and got.dtype == src.dtype and got.data_ptr() != src.data_ptr()
            bad = np.argwhere(_bits(got) != want)
            assert bad.size == 0, f"{shape} {fmt} {pattern} {kind} {table}: {len(bad)} values differ, first at {bad[:3].tolist()}"
            assert torch.equal(src, before) and torch.equal(gd, keep), "an argument was modified"
            if pattern in ("none", "all"):
                assert torch.equal(got, src)                         # nothing to fill / nothing to fill from: equal bits
            if table == 10.0 and kind == "random":                  # sigma is the table range_table(sigma)
                assert torch.equal(fill_holes_guided(src, gd, s, 10.0, None if top == 255 else top), got)


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_constant_table_is_the_plain_filler_on_the_device(shape):
    s = R.SHAPE_SCALE[shape]
    gd = _guide_dev(shape, s, "random")
    flat = _guide_dev(shape, s, "constant")
    for top in F.MAXIMA:
        dm = None if top == 255 else top
        for pattern in F.PATTERNS:
            src = _codes_dev(F.case(shape, pattern, top))
            plain = fill_holes(src, dm)
            for c in ("c1", "c37", "c256"):
                assert torch.equal(fill_holes_guided(src, gd, s, depth_max=dm, _table=_table_dev(c)), plain), (top, pattern, c)
            assert torch.equal(fill_holes_guided(src, flat, s, 10.0, dm), plain), (top, pattern, "constant guide")


def test_plane_forms_views_and_alignments():
    """(h, w) planes with (H, W) guides, uint16 tensors, and guides that start at every byte alignment inside a larger image:
    the 16-byte, the 4-byte and the byte path of the guidance reduction give the same bits."""
    shape, s = (3, 9, 13), 8
    codes, g = F.case(shape, "levels", 65535), R.guide_case(shape, s, "scene")
    want = R.want(shape, "levels", 65535, s, "scene", 10.0)
    dev = _codes_dev(codes)
    one = fill_holes_guided(dev[1], torch.from_numpy(g[1].copy()).cuda(), s)
    assert one.shape == (9, 13) and one.dtype == torch.int16 and np.array_equal(_bits(one), want[1])
    u16 = fill_holes_guided(dev.view(torch.uint16), torch.from_numpy(g.copy()).cuda(), s)
    assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want)
    B, H, W = g.shape
    for dy, dx, pad in ((0, 0, 8), (0, 16, 24), (1, 4, 12), (2, 3, 5), (0, 1, 0), (3, 2, 9)):
        big = np.full((B, H + dy + 1, W + dx + pad), 77, dtype=np.uint8)
        big[:, dy:dy + H, dx:dx + W] = g
        view = torch.from_numpy(big).cuda()[:, dy:, dx:]
        got = fill_holes_guided(dev, view, s)
        assert np.array_equal(_bits(got), want), (dy, dx, pad)
    wide, sw = (1, 70, 200), 4                                       # three launches, a guide off every alignment
    gw = R.guide_case(wide, sw, "random")
    big = np.zeros((1, 281, 803), dtype=np.uint8)
    big[:, 1:, 3:] = gw
    got = fill_holes_guided(_codes_dev(F.case(wide, "levels", 255)), torch.from_numpy(big).cuda()[:, 1:, 3:], sw)
    assert np.array_equal(_bits(got), R.want(wide, "levels", 255, sw, "random", 10.0))
    with pytest.raises(ValueError, match="smaller than the 72x104"):
        fill_holes_guided(dev, torch.zeros(3, 72, 103, dtype=torch.uint8, device="cuda"), s)
    with pytest.raises(ValueError, match="2 guidance images for 3 maps"):
        fill_holes_guided(dev, torch.zeros(2, 72, 104, dtype=torch.uint8, device="cuda"), s)
    with pytest.raises(ValueError, match="unit stride along a row"):
        fill_holes_guided(dev, torch.zeros(3, 72, 208, dtype=torch.uint8, device="cuda")[:, :, ::2], s)
    with pytest.raises(RuntimeError, match="expects a uint8 guide"):
        fill_holes_guided(dev, torch.zeros(3, 72, 104, device="cuda"), s)


@pytest.mark.parametrize("s", [8, 16])
def test_tiles_at_the_other_scales(s):
    """The four-tile plane at x8 and x16 (test_equals_the_restatement runs it at x4): every tile's guidance reduction at the
    other two segment widths, the last tile's partial width included."""
    shape = (1, 70, 200)
    gd = torch.from_numpy(R.guide_case(shape, s, "random").copy()).cuda()
    for pattern in ("levels", "cross"):
        got = fill_holes_guided(_codes_dev(F.case(shape, pattern, 65535)), gd, s)
        assert np.array_equal(_bits(got), R.want(shape, pattern, 65535, s, "random", 10.0)), (s, pattern)


def test_two_streams_same_bits():
    for shape in ((2, 64, 64), (1, 70, 200)):
        s = R.SHAPE_SCALE[shape]
        want = R.want(shape, "levels", 65535, s, "scene", 10.0)
        dev, gd = _codes_dev(F.case(shape, "levels", 65535)), _guide_dev(shape, s, "scene")
        range_table(10.0, dev.device)
        torch.cuda.synchronize()
        outs = []
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        for st in streams:
            with torch.cuda.stream(st):
                outs.append(fill_holes_guided(dev, gd, s))
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and np.array_equal(_bits(outs[0]), want)


def test_refusals_leave_out_untouched():
    lib = L.load()
    B, h, w, s = 1, 5, 7, 4
    src = _codes_dev(F.case((B, h, w), "cross", 65535))
    gd = _guide_dev((B, h, w), s, "random")[:, :20, :28].contiguous()
    gd2 = torch.cat([gd, gd])                                        # (the refusal of a short image stride names two images)
    tab = _table_dev(10.0)
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((2, h, w), -21555, dtype=torch.int16, device="cuda")
    keep_src = src.clone()

    def call(B=B, h=h, w=w, src=src.data_ptr(), fmt=L.FILL_U16, top=65535, guide=gd2.data_ptr(), row_bytes=28, image_bytes=560,
             scale=s, tab=tab.data_ptr(), out=out.data_ptr(), ws=ws.data_ptr(), ws_bytes=None):
        need = B * lib.codon_fill_guided_workspace_bytes(h, w) if B > 0 else 0
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_fill_holes_guided(B, h, w, p(src), fmt, top, p(guide), row_bytes, image_bytes, scale, p(tab), p(out), p(ws),
                                         ws_bytes, ops._stream(torch.device("cuda:0")))
        return st, lib.codon_last_error_string().decode()

    for kw, word in R.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("fill_holes_guided: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="fill_holes_guided failed with status -1: fill_holes_guided: "):
            L.check(st, "fill_holes_guided")
    assert "unaligned" in call(src=src.data_ptr() + 1)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and torch.equal(src, keep_src)
    assert call()[0] == 0                                            # and the good call they all differ from goes through
    assert np.array_equal(_bits(out[0]), R.want((B, h, w), "cross", 65535, s, "random", 10.0)[0]) and (out[1] == -21555).all()


# ---- the end-to-end tie: training's pool and inference's input --------------------------------------------------------------------

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
def test_trainset_of_guided_filled_maps(tmp_path, s, bits, levels):
    """TrainSet(lr_dir=, fill_holes=True, fill_guided=True): the pool's low-resolution planes are the restatement's guided fill
    of the files with the records' guides, nothing else in the pool moves, and synthesize's x is the D4 window of
    codes_to_input(fill_holes_guided(whole file)) -- one launch, no host synchronisation."""
    recs, rows = T.case(s, levels)
    dd, cd, ld = T.write_set(str(tmp_path), recs, bits)
    kw = dict(depth_bits=bits, depth_max=levels if bits == 16 else 65535, lr_dir=ld, scale=s)
    ts = train.TrainSet(dd, cd, "cuda:0", fill_holes=True, fill_guided=True, fill_sigma=6.0, **kw)
    plain = train.TrainSet(dd, cd, "cuda:0", fill_holes=True, **kw)
    assert ts.fill_holes and ts.fill_guided and ts.fill_sigma == 6.0 and plain.fill_holes and not plain.fill_guided
    tab = R.range_table(6.0)
    want = T.pack([(d, g, R.fill_plane(lr, g, s, tab)) for d, g, lr in recs], bits)[0]
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
    px, py, pt = train.synthesize(plain, descs, s, P, fill_holes=True)
    assert torch.equal(y, py) and torch.equal(t, pt) and not torch.equal(x, px)
    dm = levels if bits == 16 else None
    whole = [infer.codes_to_input(fill_holes_guided(_codes_dev(lr), torch.from_numpy(g.copy()).cuda(), s, 6.0, dm), s,
                                  torch.float32, dm)[0, 0] for _, g, lr in recs]
    for b, (i, H, W, y0, x0, op) in enumerate(rows):
        assert whole[i].shape == (H, W)
        assert torch.equal(x[b, 0], _d4(whole[i][y0:y0 + P, x0:x0 + P], op)), (b, i, y0, x0, op)
    with pytest.raises(ValueError, match="fit: fill_guided False with a TrainSet built with fill_guided True"):
        train.fit(None, ts, 1, scale=s, crop=P, batch=1, fill_holes=True)


class _Capture:
    """Stands in for the network in run_loop: keeps the depth input it was given and returns it."""

    def __init__(self):
        self.x = []

    def __call__(self, x, y):
        self.x.append(x)
        return x


def _write_scene(root, bits, depth_max, s):
    """lr/ and color/ with two occlusion scenes (the second's guidance larger than the map needs): (lr dir, color dir, cases)"""
    lrd, cd = os.path.join(root, "lr"), os.path.join(root, "color")
    os.makedirs(lrd)
    os.makedirs(cd)
    top = 255 if bits == 8 else depth_max
    cases = []
    for i, (h, w, pad) in enumerate([(12, 17, 0), (9, 13, 3)]):
        codes, guide, _ = R.scene(h, w, s, top, seed=3 + i)
        big = np.full((h * s + pad, w * s + 2 * pad), 9, dtype=np.uint8)
        big[:h * s, :w * s] = guide
        (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(lrd, f"{i:02d}.png"), codes)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), big)
        cases.append((codes, guide))
    return lrd, cd, cases


@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
def test_run_loop_builds_the_guided_input(tmp_path, bits, depth_max):
    """run_loop(lr_depth=, fill_holes=True, fill_guided=True) with a stand-in network that returns its input: both loops, f32 and
    f16, give codes_to_input of the restatement's guided fill; pipelined equals serial byte for byte (the outputs written, too);
    the result differs from the run without fill_guided; normalize composes behind the filling."""
    s, sigma = 4, 7.0
    lrd, cd, cases = _write_scene(str(tmp_path), bits, depth_max, s)
    dev = torch.device("cuda:0")
    dm = depth_max if bits == 16 else None
    kw = dict(emit=quiet, depth_bits=bits, depth_max=depth_max if bits == 16 else 65535, lr_depth=lrd, scale=s, fill_holes=True)
    tab = R.range_table(sigma)
    for tdt in (torch.float32, torch.float16):
        want = [infer.codes_to_input(_codes_dev(R.fill_plane(c, g, s, tab)), s, tdt, dm) for c, g in cases]
        xs, files = {}, {}
        for pipelined in (False, True):
            m = _Capture()
            od = tmp_path / f"out_{tdt}_{pipelined}"
            os.makedirs(od)
            r = infer.run_loop(m, dev, tdt, None, cd, None, str(od), pipelined=pipelined, fill_guided=True, fill_sigma=sigma, **kw)
            assert r["n"] == 2 and len(m.x) == 2
            for got, ref in zip(m.x, want):
                assert got.dtype == tdt and got.shape == ref.shape and np.array_equal(_bits(got), _bits(ref)), (tdt, pipelined)
            xs[pipelined] = m.x
            files[pipelined] = {n: open(od / n, "rb").read() for n in sorted(os.listdir(od))}
        assert len(files[True]) == 2 and files[True] == files[False]
        m = _Capture()
        infer.run_loop(m, dev, tdt, None, cd, None, None, pipelined=False, **kw)
        assert all(not torch.equal(a, b) for a, b in zip(m.x, xs[False]))          # the option reaches the network's input
    from codon_amd.upsample import stretch_codes
    m = _Capture()
    infer.run_loop(m, dev, torch.float32, None, cd, None, None, fill_guided=True, fill_sigma=sigma, normalize=True, **kw)
    for got, (c, g) in zip(m.x, cases):
        ref = infer.codes_to_input(stretch_codes(_codes_dev(R.fill_plane(c, g, s, tab)), dm)[0], s, torch.float32, dm)
        assert torch.equal(got, ref)
    with pytest.raises(ValueError, match="smaller than the"):
        small = tmp_path / "small"
        os.makedirs(small)
        for n in ("00.png", "01.png"):
            io.write_gray(str(small / n), np.zeros((20, 20), dtype=np.uint8))
        infer.run_loop(_Capture(), dev, torch.float32, None, str(small), None, None, pipelined=False, fill_guided=True, **kw)


def test_launch_sequences(tmp_path):
    """Without the option run_loop issues the calls it always did -- codon_fill_holes ahead of codon_lr_codes_to_input and not
    one call more; with it that one call becomes codon_fill_holes_guided and nothing else changes."""
    from tests.abi_log_8bit import _acl
    lrd, cd, _ = _write_scene(str(tmp_path), 8, 255, 4)
    dev = torch.device("cuda:0")
    kw = dict(emit=quiet, lr_depth=lrd, scale=4, pipelined=False)
    for extra in ({}, {"fill_holes": True}, {"fill_holes": True, "fill_guided": True}):
        infer.run_loop(_Capture(), dev, torch.float32, None, cd, None, None, **kw, **extra)          # tables and workspaces
    torch.cuda.synchronize()
    real = L.load()
    names = {}
    try:
        for key, extra in (("off", {}), ("plain", {"fill_holes": True}), ("guided", {"fill_holes": True, "fill_guided": True})):
            log = _acl().install()
            try:
                infer.run_loop(_Capture(), dev, torch.float32, None, cd, None, None, **kw, **extra)
            finally:
                L._lib = real
            names[key] = [n for n, _, _ in log if not n.endswith("_workspace_bytes")]
            if key == "guided":
                args = next(a for n, a, _ in log if n == "codon_fill_holes_guided")
                assert args[:3] == [1, 12, 17] and args[4:6] == [L.FILL_U8, 255] and args[7:10] == [68, 0, 4]
    finally:
        L._lib = real
    assert "codon_lr_codes_to_input" in names["off"] and not any("fill" in n for n in names["off"])
    want = []
    for n in names["off"]:
        want += ["codon_fill_holes", n] if n == "codon_lr_codes_to_input" else [n]
    assert names["plain"] == want and len(want) == len(names["off"]) + 2
    assert names["guided"] == [n + "_guided" if n == "codon_fill_holes" else n for n in want]


def test_infer_cli_pipelined_equals_serial(tmp_path, capsys):
    from codon_amd import CODONNet
    lrd, cd, _ = _write_scene(str(tmp_path), 8, 255, 4)
    names = sorted(os.listdir(lrd))
    torch.manual_seed(5)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 2, "model": CODONNet()}, ck)
    outs = {}
    for mode in ("serial", "pipe", "plain", "sigma"):
        od = tmp_path / f"out_{mode}"
        capsys.readouterr()
        rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--out", str(od), "--weights", ck, "--dtype", "f32",
                         "--fill-holes"] + (["--serial"] if mode == "serial" else []) + ([] if mode == "plain" else ["--fill-guided"])
                        + (["--fill-sigma", "2.5"] if mode == "sigma" else []))
        assert rc == 0
        outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in names})
    assert outs["serial"] == outs["pipe"]
    assert all(outs["plain"][1][n] != outs["pipe"][1][n] for n in names)           # the option reaches the network's input
    assert any(outs["sigma"][1][n] != outs["pipe"][1][n] for n in names)           # and so does its sigma
    capsys.readouterr()


def test_fit_keeps_the_keys_and_validates_guided(tmp_path):
    """train.main with --train-lr-depth --fill-holes --fill-guided: the checkpoint carries both keys, a resume with the option
    flipped is refused by name before any GPU work, and validation fills as inference does."""
    recs, _ = T.case(4, 255)
    dd, cd, ld = T.write_set(str(tmp_path), recs, 8)
    cli = lambda *extra: ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--train-lr-depth", ld, "--fill-holes",     # noqa: E731
                          "--crop", "16", "--batch", "2", "--log-every", "1", "--seed", "5", "--dtype", "bf16", *extra]
    a, b = str(tmp_path / "a.pth"), str(tmp_path / "b.pth")
    on = train.main(cli("--fill-guided", "--fill-sigma", "6", "--steps", "2", "--save", a), emit=quiet)
    off = train.main(cli("--steps", "2", "--save", b), emit=quiet)
    ca, cb = torch.load(a, weights_only=False)["args"], torch.load(b, weights_only=False)["args"]
    assert ca["fill_guided"] is True and ca["fill_sigma"] == 6.0 and ca["fill_holes"] is True
    assert "fill_guided" not in cb and "fill_sigma" not in cb                       # a run without the option keeps its keys
    assert all(np.isfinite(v) for _, v in on["losses"]) and on["losses"] != off["losses"]
    with pytest.raises(ValueError, match="fill_guided True != False"):
        train.main(cli("--steps", "4", "--resume", a), emit=quiet)
    with pytest.raises(ValueError, match="fill_guided False != True"):
        train.main(cli("--fill-guided", "--steps", "4", "--resume", b), emit=quiet)
    with pytest.raises(ValueError, match="fill_sigma 6.0 != 10.0"):
        train.main(cli("--fill-guided", "--steps", "4", "--resume", a), emit=quiet)
    from codon_amd import CODONNet
    torch.manual_seed(1)
    m = CODONNet().cuda()
    dev = torch.device("cuda:0")
    val = {"lr_depth": ld, "scale": 4, "color": cd, "label": dd, "every": 1, "fill_holes": True}
    r = train.validate(m, dev, dict(val, fill_guided=True, fill_sigma=6.0), emit=quiet)
    r0 = train.validate(m, dev, val, emit=quiet)
    m.eval()
    with torch.no_grad():
        want = infer.run_loop(m, dev, torch.float32, None, cd, dd, emit=quiet, lr_depth=ld, scale=4, fill_holes=True,
                              fill_guided=True, fill_sigma=6.0)
    assert r["n"] == len(recs) and (r["rmse_mean"], r["ssim_mean"]) == (want["rmse_mean"], want["ssim_mean"])
    assert (r0["rmse_mean"], r0["ssim_mean"]) != (r["rmse_mean"], r["ssim_mean"])
