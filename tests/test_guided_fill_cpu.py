"""The guidance-aware pull-push hole filler without a GPU: what the definition promises, asserted on the numpy
restatement (tests/guided_fill_ref.py) over every shape, pattern and maximum of the plain filler's tests; that a constant
guidance image or a constant table gives the plain filler's bits; a case worked by hand; the occlusion scene, on which the
guided fill must at least halve the plain fill's error over the holes; the host-side workspace helper and refusals of the C
entry; the range table; the command lines' refusals and defaults; and a resume of a checkpoint written before the option
existed."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, train, upsample
from tests import fill_ref as F
from tests import guided_fill_ref as R


# ---- the definition ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", [3.0, 10.0])
@pytest.mark.parametrize("s", R.SCALES)
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_consequences_of_the_definition(shape, s, sigma):
    for pattern in F.PATTERNS:
        for top in F.MAXIMA:
            codes, filled = F.case(shape, pattern, top), R.want(shape, pattern, top, s, "random", sigma)
            for c, f in zip(codes, filled):
                F.check_consequences(c, f, top)


@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_constant_guide_or_table_is_the_plain_fill(shape):
    s = R.SHAPE_SCALE[shape]
    for pattern in F.PATTERNS:
        for top in F.MAXIMA:
            plain = F.want(shape, pattern, top)
            assert np.array_equal(R.want(shape, pattern, top, s, "constant", 10.0), plain), (pattern, top, "constant guide")
            assert np.array_equal(R.want(shape, pattern, top, s, "random", "c37"), plain), (pattern, top, "constant table")
            assert np.array_equal(R.want(shape, pattern, top, s, "random", "c256"), plain), (pattern, top, "constant table")
    codes = F.case((3, 9, 13), "cross", 10000)                      # and the guidance does matter otherwise
    assert not np.array_equal(R.want((3, 9, 13), "cross", 10000, 8, "random", 3.0), F.want((3, 9, 13), "cross", 10000))
    assert (codes == 0).any()


def test_by_hand():
    """3 x 3 codes at x4, guidance 200 on the left two columns of pixels and 40 on the right one, T = range_table(10):
    T[0] = 256, T[53] = T[107] = T[160] = 1."""
    T = R.range_table(10.0)
    assert T[0] == 256 and T[53] == 1 and T[107] == 1 and T[160] == 1 and T[10] == 155
    c = np.array([[100, 0, 0], [0, 0, 0], [0, 0, 20]], dtype=np.uint8)
    g = np.full((12, 12), 200, dtype=np.uint8)
    g[:, 8:] = 40
    G0 = R.guide_base(g, 3, 3, 4)
    assert G0.tolist() == [[200, 200, 40]] * 3
    # level 1 (2 x 2): G the means over the children inside: [[200, 40], [200, 40]]; V: [[100, 0], [0, 20]]; A where V is valid:
    # A_1(0,0) = 200 (from the pixel (0,0)), A_1(1,1) = 40 (from the pixel (2,2))
    G1 = R.pull_guide(G0)
    V1 = F.pull(c.astype(np.int64))
    A1 = R.pull_attached(c.astype(np.int64), np.where(c != 0, G0, 0))
    assert G1.tolist() == [[200, 40], [200, 40]] and V1.tolist() == [[100, 0], [0, 20]] and A1.tolist() == [[200, 0], [0, 40]]
    # level 2 (1 x 1): V = (2 * 120 + 2) // 4 = 60, A = (2 * 240 + 2) // 4 = 120, G = (2 * 480 + 4) // 8 = 120
    assert F.pull(V1).tolist() == [[60]] and R.pull_attached(V1, A1).tolist() == [[120]] and R.pull_guide(G1).tolist() == [[120]]
    # F_1: every parent of a level-1 hole is the one top cell: the weights cancel, 60 everywhere there
    F1 = R.push(V1, G1, F.pull(V1), F.pull(V1), R.pull_attached(V1, A1), R.pull_guide(G1), T)
    assert F1.tolist() == [[100, 60], [60, 20]]
    f = R.fill_plane(c, g, 4, T)
    # F_0(0,1): G 200; parents py 0 qy 0, px 0 qx 1 -> (0,0) F 100 A^ 200 (valid) weights 9 and 3; (0,1) F 60 A^ G_1 = 40 (a
    # hole) weights 3 and 1: w = 12 * T[0] = 3072 and 4 * T[160] = 4 -> (2 * (3072 * 100 + 4 * 60) + 3076) // (2 * 3076) = 100
    assert f[0, 1] == (2 * (3072 * 100 + 4 * 60) + 3076) // (2 * 3076) == 100
    # the plain filler's value there is (9 * 100 + 3 * 60 + 3 * 100 + 60 + 8) >> 4 = 90
    assert F.fill_plane(c)[0, 1] == 90
    # F_0(1,2): G 40; py 0 qy 1 (y odd), px 1 qx 0 (x even): (0,1) F 60 A^ 40 w 9 * 256; (0,0) F 100 A^ 200 w 3 * T[160] = 3;
    # (1,1) F 20 A^ 40 w 3 * 256; (1,0) F 60 A^ G_1 = 200 w 1
    num, den = 2304 * 60 + 3 * 100 + 768 * 20 + 60, 2304 + 3 + 768 + 1
    assert f[1, 2] == (2 * num + den) // (2 * den) == 50
    assert f[0, 0] == 100 and f[2, 2] == 20
    # 32 bits hold everything: the four parents at the largest code and the largest weights
    assert R.NUMERATOR_MAX == 2 * 4096 * 65535 + 4096 < 1 << 31
    top = np.array([[65535, 0], [0, 65535]], dtype=np.uint16)
    assert (R.fill_plane(top, np.zeros((8, 8), dtype=np.uint8), 4, np.full(256, 256, dtype=np.uint16)) == 65535).all()


@pytest.mark.parametrize("h, w, s, top", [(48, 64, 4, 255), (48, 64, 8, 10000), (70, 200, 4, 65535), (33, 47, 16, 255)])
def test_occlusion_scene(h, w, s, top):
    """At sigma 10 the guided fill's mean absolute error over the holes is at most half of the plain fill's."""
    codes, guide, truth = R.scene(h, w, s, top)
    holes = codes == 0
    assert 0.05 < holes.mean() < 0.5 and guide.shape == (h * s, w * s)
    plain = R.hole_error(F.fill_plane(codes), codes, truth)
    guided = R.hole_error(R.fill_plane(codes, guide, s, R.range_table(10.0)), codes, truth)
    print(f"{h}x{w} x{s} top {top}: plain {plain / top:.4f} guided {guided / top:.4f} of full scale, ratio {guided / plain:.3f}")
    assert guided <= 0.5 * plain


# ---- the C entry points, on the host ---------------------------------------------------------------------------------------------

def test_workspace_bytes_without_gpu():
    lib = L.load()
    for h, w in [s[1:] for s in F.SHAPES] + [(93, 116), (120, 160), (4096, 4096), (4096, 1), (1, 4096), (64, 65)]:
        got = lib.codon_fill_guided_workspace_bytes(h, w)
        need = R.workspace_bytes(h, w)
        assert need == 4 * sum(a * b for a, b in F.levels(h, w)[1:]) + h * w
        assert got >= need and got > 0 and got % 16 == 0 and got < need + 16, (h, w, got, need)
    for h, w in ((0, 5), (5, 0), (-1, 5), (4097, 5), (5, 4097)):
        assert lib.codon_fill_guided_workspace_bytes(h, w) == 0, (h, w)


def test_refusals_without_gpu():
    lib = L.load()
    fake, other, third, fourth, fifth = 4096, 1 << 20, 1 << 21, 1 << 22, 1 << 23   # never dereferenced: every call is refused

    def call(B=1, h=5, w=7, src=fake, fmt=L.FILL_U16, top=65535, guide=fourth, row_bytes=28, image_bytes=0, scale=4, tab=fifth,
             out=other, ws=third, ws_bytes=None):
        need = B * lib.codon_fill_guided_workspace_bytes(h, w) if B > 0 else 0
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else C.c_void_p(v)               # noqa: E731
        st = lib.codon_fill_holes_guided(B, h, w, p(src), fmt, top, p(guide), row_bytes, image_bytes, scale, p(tab), p(out), p(ws),
                                         ws_bytes, None)
        return st, lib.codon_last_error_string().decode()

    for kw, word in R.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("fill_holes_guided: ") and word in msg, (kw, msg)
    assert call(src=fake + 1)[1] == "fill_holes_guided: unaligned plane, table or workspace"
    assert call(ws=third + 8)[1] == "fill_holes_guided: unaligned plane, table or workspace"
    assert call(tab=fifth + 1)[1] == "fill_holes_guided: unaligned plane, table or workspace"
    assert "guide images" not in call(B=1, image_bytes=-5, ws_bytes="short")[1]      # one image: the image stride is not looked at


def test_range_table():
    for sigma in (0.5, 3.0, 10.0, 40.0, 1000.0):
        t = upsample.range_table(sigma)
        d = np.arange(256, dtype=np.float64)
        want = np.maximum(1.0, np.rint(256.0 * np.exp(-d * d / (2.0 * sigma * sigma))))
        assert t.shape == (256,) and t.dtype == np.uint16 and np.array_equal(t, want) and np.array_equal(t, R.range_table(sigma))
        assert t[0] == 256 and (np.diff(t.astype(np.int64)) <= 0).all() and t.min() >= 1 and t.max() == 256
        assert not t.flags.writeable
    assert upsample.range_table() is upsample.range_table(10.0) and upsample.FILL_SIGMA == 10.0
    for bad in (0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError, match="fill_sigma"):
            upsample.range_table(bad)


# ---- the command lines ------------------------------------------------------------------------------------------------------------

def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_cli_refusals_and_defaults(capsys):
    lr = ["--lr-depth", "d", "--input-color", "c"]
    for argv, word in ((lr + ["--fill-guided"], "--fill-guided needs --fill-holes"),
                       (["--input-depth", "d", "--input-color", "c", "--fill-guided"], "--fill-guided needs --fill-holes"),
                       (lr + ["--fill-holes", "--fill-sigma", "5"], "--fill-sigma needs --fill-guided"),
                       (lr + ["--fill-holes", "--fill-guided", "--fill-sigma", "0"], "--fill-sigma 0.0 must be positive"),
                       (lr + ["--fill-holes", "--fill-guided", "--fill-sigma", "-2"], "--fill-sigma -2.0 must be positive")):
        with pytest.raises(SystemExit):
            infer.main(argv)
        assert word in capsys.readouterr().err
    for argv, word in ((_argv("--degrade-holes", "--fill-holes", "--fill-guided"),
                        "--fill-guided is refused with --degrade-holes: the synthetic path holds its guidance as fp32 D4 crops"),
                       (_argv("--train-lr-depth", "l", "--fill-guided"), "--fill-guided needs --train-lr-depth --fill-holes"),
                       (_argv("--fill-guided"), "--fill-guided needs --train-lr-depth --fill-holes"),
                       (_argv("--train-lr-depth", "l", "--fill-holes", "--fill-sigma", "4"), "--fill-sigma needs --fill-guided"),
                       (_argv("--train-lr-depth", "l", "--fill-holes", "--fill-guided", "--fill-sigma", "0"), "must be positive")):
        with pytest.raises(SystemExit):
            train.parse_args(argv)
        assert word in capsys.readouterr().err
    assert train.GUIDED_DEFAULTS == {"fill_guided": False, "fill_sigma": 10.0} and train.FILL_DEFAULTS == {"fill_holes": False}
    for extra in ((), ("--degrade-holes", "--fill-holes"), ("--train-lr-depth", "l", "--fill-holes")):
        a = train.parse_args(_argv(*extra))
        assert a.fill_guided is False and not {"fill_guided", "fill_sigma"} & set(train.run_args(a))
    a = train.parse_args(_argv("--train-lr-depth", "l", "--fill-holes", "--fill-guided"))
    assert a.fill_guided is True and a.fill_sigma == 10.0
    r = train.run_args(a)
    assert r["fill_guided"] is True and r["fill_sigma"] == 10.0 and r["fill_holes"] is True
    plain = train.run_args(train.parse_args(_argv("--train-lr-depth", "l", "--fill-holes")))
    assert set(r) - set(plain) == {"fill_guided", "fill_sigma"} and all(r[k] == v for k, v in plain.items())
    assert train.run_args(train.parse_args(_argv("--train-lr-depth", "l", "--fill-holes", "--fill-guided", "--fill-sigma", "4.5")))[
        "fill_sigma"] == 4.5
    with pytest.raises(ValueError, match="run_loop: fill_guided needs fill_holes"):
        infer.run_loop(None, None, torch.float32, None, "c", lr_depth="d", scale=4, fill_guided=True)
    with pytest.raises(ValueError, match="run_loop: fill_sigma 0"):
        infer.run_loop(None, None, torch.float32, None, "c", lr_depth="d", scale=4, fill_holes=True, fill_guided=True, fill_sigma=0)


def _write_set(root):
    g = np.random.default_rng(1)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "lr")]
    for d in dirs:
        os.makedirs(d)
    io.write_gray(os.path.join(dirs[0], "00.png"), g.integers(1, 256, size=(40, 48)).astype(np.uint8))
    io.write_gray(os.path.join(dirs[1], "00.png"), g.integers(0, 256, size=(40, 48)).astype(np.uint8))
    io.write_gray(os.path.join(dirs[2], "00.png"), g.integers(0, 256, size=(10, 12)).astype(np.uint8))
    return dirs


def test_python_refusals(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path))
    with pytest.raises(ValueError, match="TrainSet: fill_guided needs fill_holes"):
        train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4, fill_guided=True)
    with pytest.raises(ValueError, match="TrainSet: fill_holes needs lr_dir"):
        train.TrainSet(dd, cd, "cpu", fill_holes=True, fill_guided=True)
    tl = train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4)                # low-resolution maps, loaded WITHOUT filling
    assert tl.fill_guided is False and tl.fill_sigma == 10.0
    with pytest.raises(ValueError, match="fit: fill_guided True .* with a TrainSet built with fill_guided False"):
        train.fit(None, tl, 1, scale=4, crop=32, batch=1, fill_guided=True)
    ts = train.TrainSet(dd, cd, "cpu")
    with pytest.raises(ValueError, match="fit: fill_guided True .* with a TrainSet built with fill_guided False"):
        train.fit(None, ts, 1, scale=4, crop=32, batch=1, degrade_holes=True, fill_holes=True, fill_guided=True)
    tl.prep = dataclasses.replace(tl.prep, fill_holes=True, fill_guided=True)         # as if it had been built with both, at sigma 10
    with pytest.raises(ValueError, match="fit: fill_guided False with a TrainSet built with fill_guided True"):
        train.fit(None, tl, 1, scale=4, crop=32, batch=1, fill_holes=True)
    with pytest.raises(ValueError, match=r"fit: fill_guided True \(fill_sigma 3.0\) with a TrainSet built with fill_guided True "
                                         r"\(fill_sigma 10.0\)"):
        train.fit(None, tl, 1, scale=4, crop=32, batch=1, fill_holes=True, fill_guided=True, fill_sigma=3.0)
    f = upsample.fill_holes_guided
    u8 = torch.zeros(4, 5, dtype=torch.uint8)
    gd = torch.zeros(16, 20, dtype=torch.uint8)
    for bad in (torch.zeros(3, dtype=torch.uint8), torch.zeros(2, 3, 4, 5, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.int32),
                torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(RuntimeError, match="fill_holes_guided expects"):
            f(bad, gd, 4)
    with pytest.raises(ValueError, match="depth_max 1000 with 8-bit codes"):
        f(u8, gd, 4, depth_max=1000)
    with pytest.raises(ValueError, match=r"scale 2 \(4, 8 or 16\)"):
        f(u8, gd, 2)


def test_resume_of_a_checkpoint_without_the_keys(tmp_path):
    """A checkpoint written before the option existed resumes under the defaults, and is refused by name when the option is
    flipped either way or the sigma differs."""
    base = ("--train-lr-depth", "l", "--fill-holes")
    args = train.run_args(train.parse_args(_argv(*base)))
    assert "fill_guided" not in args and "fill_sigma" not in args
    path = str(tmp_path / "old.pth")
    torch.save({"epoch": 2, "model": {}, "optimizer": {}, "rng": {}, "args": dict(args)}, path)
    assert train.load_resume(path, args)["epoch"] == 2
    guided = train.run_args(train.parse_args(_argv(*base, "--fill-guided")))
    with pytest.raises(ValueError, match="fill_guided False != True"):
        train.load_resume(path, guided)
    torch.save({"epoch": 2, "model": {}, "optimizer": {}, "rng": {}, "args": dict(guided)}, path)
    assert train.load_resume(path, guided)["epoch"] == 2
    with pytest.raises(ValueError, match="fill_guided True != False"):
        train.load_resume(path, args)
    with pytest.raises(ValueError, match="fill_sigma 10.0 != 4.0"):
        train.load_resume(path, train.run_args(train.parse_args(_argv(*base, "--fill-guided", "--fill-sigma", "4"))))
