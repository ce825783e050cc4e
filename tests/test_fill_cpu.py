"""The pull-push hole filler without a GPU: what the definition promises, asserted on the numpy restatement
(tests/fill_ref.py) over every shape, pattern and maximum of the GPU tests; the exact round trip of the fp32-on-the-grid format
for every code; the level coverage of the "levels" pattern; the host-side workspace helper and refusals of the C entry; the
command lines' refusals and defaults; and a resume of a checkpoint written before the option existed."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, train
from codon_amd.upsample import lut16, u8_lut
from tests import fill_ref as F


# ---- the definition ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("top", F.MAXIMA)
@pytest.mark.parametrize("shape", F.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_consequences_of_the_definition(shape, top):
    for pattern in F.PATTERNS:
        codes, filled = F.case(shape, pattern, top), F.want(shape, pattern, top)
        assert codes.dtype == (np.uint8 if top == 255 else np.uint16) and codes.max(initial=0) <= top
        holes = int((codes == 0).sum())
        if pattern in ("none", "all"):
            assert holes == (0 if pattern == "none" else codes.size)
        elif min(shape[1:]) >= 5:                                   # (a 1 x 1 plane is one pixel whatever the pattern says)
            assert 0 < holes < codes.size, (pattern, holes)
        if pattern == "one":
            assert ((codes != 0).sum(axis=(1, 2)) == 1).all()
        for c, f in zip(codes, filled):
            F.check_consequences(c, f, top)
        again = F.fill(filled)                                      # a filled plane has no hole left (or only holes): unchanged
        assert np.array_equal(again, filled)


def test_by_hand():
    """3 x 3 with one valid code in a corner and one in the middle of the far edge: every step written out."""
    c = np.array([[10, 0, 0], [0, 0, 0], [0, 20, 0]], dtype=np.uint8)
    # level 1 (2 x 2): [[10, 0], [20, 0]]; level 2 (1 x 1): (2 * 30 + 2) // 4 = 15
    assert F.pull(c.astype(np.int64)).tolist() == [[10, 0], [20, 0]] and F.pull(F.pull(c.astype(np.int64))).tolist() == [[15]]
    # F_1 = [[10, 15], [20, 15]]; F_0(0,1): py 0 qy 0, px 0 qx 1 (x odd) -> (9*10 + 3*15 + 3*10 + 15 + 8) >> 4 = 11
    f, anc = F.fill_plane(c, with_levels=True)
    assert f[0, 1] == (9 * 10 + 3 * 15 + 3 * 10 + 15 + 8) >> 4 == 11
    # F_0(1,2): py 0 qy 1 (y odd), px 1 qx 0 (x even) -> (9*15 + 3*10 + 3*15 + 20 + 8) >> 4 = 14
    assert f[1, 2] == (9 * 15 + 3 * 10 + 3 * 15 + 20 + 8) >> 4 == 14
    assert f[0, 0] == 10 and f[2, 1] == 20
    assert anc.tolist() == [[0, 1, 2], [1, 1, 2], [1, 0, 2]]
    # a half is rounded up: the mean of 1 and 2 is 2
    assert F.pull(np.array([[1, 2]], dtype=np.int64)).tolist() == [[2]]
    # 32 bits hold everything: four children and four parents at the largest code
    assert 2 * 4 * 65535 + 4 < 1 << 31 and 16 * 65535 + 8 < 1 << 31
    top = np.full((2, 2), 65535, dtype=np.uint16)
    assert F.pull(top.astype(np.int64)).tolist() == [[65535]] and np.array_equal(F.fill_plane(top), top)


@pytest.mark.parametrize("depth_max", [255, 4096, 10000, 65535])
def test_fp32_round_trip_of_every_code(depth_max):
    """rintf(tab[c] * top) == c for every code: the error of tab[c] * top is below c * 2^-23 < 0.5."""
    tab = u8_lut() if depth_max == 255 else lut16(depth_max)
    assert np.array_equal(tab[:depth_max + 1].view(np.uint32), F.table(depth_max)[:depth_max + 1].view(np.uint32))
    codes = np.arange(depth_max + 1)
    prod = tab[:depth_max + 1] * np.float32(depth_max)
    assert prod.dtype == np.float32 and np.array_equal(np.rint(prod).astype(np.int64), codes)
    assert float(np.abs(prod.astype(np.float64) - codes).max()) < 0.5 and tab[0] == 0 and (tab[1:depth_max + 1] > 0).all()
    assert np.array_equal(F.from_grid(F.to_grid(codes, depth_max), depth_max), codes)


def test_level_pattern_reaches_every_ancestor_level():
    """Among the holes of the "levels" pattern every ancestor level 1 .. K occurs: no test passes through one push level only,
    and at 70 x 200 a whole 64-wide tile is empty (filled from above level 6)."""
    for shape in ((1, 5, 7), (3, 9, 13), (1, 65, 67), (1, 70, 200)):
        K = len(F.levels(*shape[1:])) - 1
        codes = F.case(shape, "levels")
        for plane in codes:
            _, anc = F.fill_plane(plane, with_levels=True)
            counts = [int((anc == k).sum()) for k in range(K + 2)]
            print(shape, "K", K, "holes per ancestor level 1..K:", counts[1:K + 1])
            assert counts[0] == int((plane != 0).sum()) and counts[K + 1] == 0
            assert all(n > 0 for n in counts[1:K + 1]), (shape, counts)
    wide = F.case((1, 70, 200), "levels")[0]
    assert not wide[:, 128:].any() and [len(F.levels(h, w)) - 1 for h, w in ((70, 200), (65, 67), (9, 13))] == [8, 7, 4]


# ---- the C entry points, on the host ---------------------------------------------------------------------------------------------

def test_workspace_bytes_without_gpu():
    lib = L.load()
    for h, w in [s[1:] for s in F.SHAPES] + [(93, 116), (120, 160), (4096, 4096), (4096, 1), (1, 4096), (64, 65)]:
        got = lib.codon_fill_holes_workspace_bytes(h, w)
        cells = F.workspace_cells(h, w)
        assert got >= 2 * cells and got > 0 and got % 16 == 0 and got <= 2 * cells + 16, (h, w, got, cells)
    for h, w in ((0, 5), (5, 0), (-1, 5), (4097, 5), (5, 4097)):
        assert lib.codon_fill_holes_workspace_bytes(h, w) == 0, (h, w)


def test_refusals_without_gpu():
    lib = L.load()
    fake, other, third = 4096, 1 << 20, 1 << 21                           # never dereferenced: every call is refused on the host

    def call(B=1, h=5, w=7, src=fake, fmt=L.FILL_U16, tab=fake, top=65535, out=other, ws=third, ws_bytes=None):
        need = B * lib.codon_fill_holes_workspace_bytes(h, w) if B > 0 else 0
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else C.c_void_p(v)               # noqa: E731
        st = lib.codon_fill_holes(B, h, w, p(src), fmt, p(tab), top, p(out), p(ws), ws_bytes, None)
        return st, lib.codon_last_error_string().decode()

    for kw, word in F.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("fill_holes: ") and word in msg, (kw, msg)
    assert call(fmt=L.FILL_U16, src=fake + 1)[1] == "fill_holes: unaligned plane or workspace"
    assert call(fmt=L.FILL_F32, top=255, out=other + 2)[1] == "fill_holes: unaligned plane or workspace"


# ---- the command lines ------------------------------------------------------------------------------------------------------------

def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_cli_refusals_and_defaults(capsys, tmp_path):
    with pytest.raises(SystemExit):
        infer.main(["--input-depth", "d", "--input-color", "c", "--fill-holes"])
    assert "--fill-holes needs --lr-depth" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(_argv("--fill-holes"))
    assert "--fill-holes needs --train-lr-depth or --degrade-holes" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                       # a validation set alone is no companion
        train.parse_args(_argv("--fill-holes", "--val-lr-depth", "v", "--val-color", "c"))
    capsys.readouterr()
    a = train.parse_args(_argv())
    assert a.fill_holes is False and "fill_holes" not in train.run_args(a)
    assert train.FILL_DEFAULTS == {"fill_holes": False}
    for extra in (("--degrade-holes",), ("--train-lr-depth", "l")):
        a = train.parse_args(_argv("--fill-holes", *extra))
        assert a.fill_holes is True and train.run_args(a)["fill_holes"] is True
        assert "fill_holes" not in train.run_args(train.parse_args(_argv(*extra)))
    with pytest.raises(ValueError, match="run_loop: fill_holes needs lr_depth"):
        infer.run_loop(None, None, torch.float32, "d", "c", fill_holes=True)


def _write_set(root, lr=False):
    g = np.random.default_rng(1)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "lr")]
    for d in dirs:
        os.makedirs(d)
    io.write_gray(os.path.join(dirs[0], "00.png"), g.integers(1, 256, size=(40, 48)).astype(np.uint8))
    io.write_gray(os.path.join(dirs[1], "00.png"), g.integers(0, 256, size=(40, 48)).astype(np.uint8))
    if lr:
        io.write_gray(os.path.join(dirs[2], "00.png"), g.integers(0, 256, size=(10, 12)).astype(np.uint8))
    return dirs


def test_python_refusals(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path / "a"))
    with pytest.raises(ValueError, match="TrainSet: fill_holes needs lr_dir"):
        train.TrainSet(dd, cd, "cpu", fill_holes=True)
    ts = train.TrainSet(dd, cd, "cpu")
    assert ts.fill_holes is False
    descs = np.asarray([[0, 40, 48, 0, 0, 0]], dtype=np.int64)
    with pytest.raises(ValueError, match="synthesize: fill_holes needs degrade_holes"):
        train.synthesize(ts, descs, 4, 32, fill_holes=True)
    with pytest.raises(ValueError, match="fit: fill_holes needs degrade_holes"):
        train.fit(None, ts, 1, scale=4, crop=32, batch=1, fill_holes=True)
    dd, cd, ld = _write_set(str(tmp_path / "b"), lr=True)
    tl = train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4)                # low-resolution maps, loaded WITHOUT filling
    with pytest.raises(ValueError, match="synthesize: fill_holes needs degrade_holes, or a TrainSet of low-resolution maps built"):
        train.synthesize(tl, descs, 4, 32, fill_holes=True)
    with pytest.raises(ValueError, match="built with the same fill_holes"):
        train.fit(None, tl, 1, scale=4, crop=32, batch=1, fill_holes=True)
    from codon_amd.upsample import fill_holes
    for bad in (torch.zeros(3, dtype=torch.uint8), torch.zeros(2, 3, 4, 5, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.int32),
                torch.zeros(4, 5), torch.zeros(1, 2, 4, 5)):
        with pytest.raises(RuntimeError, match="fill_holes expects"):
            fill_holes(bad)
    with pytest.raises(ValueError, match="depth_max 1000 with 8-bit codes"):
        fill_holes(torch.zeros(4, 5, dtype=torch.uint8), depth_max=1000)
    with pytest.raises(ValueError):
        fill_holes(torch.zeros(4, 5, dtype=torch.int16), depth_max=0)


def test_resume_of_a_checkpoint_without_the_key(tmp_path):
    """A checkpoint written before the option existed resumes under the defaults, and is refused by name with the option."""
    a = train.parse_args(_argv("--degrade-holes"))
    args = train.run_args(a)
    assert "fill_holes" not in args
    path = str(tmp_path / "old.pth")
    torch.save({"epoch": 2, "model": {}, "optimizer": {}, "rng": {}, "args": dict(args)}, path)
    assert train.load_resume(path, args)["epoch"] == 2
    with pytest.raises(ValueError, match="fill_holes False != True"):
        train.load_resume(path, train.run_args(train.parse_args(_argv("--degrade-holes", "--fill-holes"))))
    filled = dict(args, fill_holes=True)
    torch.save({"epoch": 2, "model": {}, "optimizer": {}, "rng": {}, "args": filled}, path)
    assert train.load_resume(path, filled)["epoch"] == 2
    with pytest.raises(ValueError, match="fill_holes True != False"):
        train.load_resume(path, args)
