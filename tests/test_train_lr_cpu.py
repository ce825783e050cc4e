"""Training on real low-resolution depth maps without a GPU: the numpy restatement against the existing
restatements, the records TrainSet(lr_dir=...) packs, its refusals, the host-side refusals of codon_train_crops_lr and of the
command line, and the resume key."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import io, train
from oracle import upsample_oracle as U
from tests import resample_masked_ref as M
from tests import train_data_ref as R
from tests import train_lr_ref as T

SCALES = (4, 8, 16)


@pytest.mark.parametrize("levels", [255, 4096])
@pytest.mark.parametrize("s", SCALES)
def test_hole_free_planes_give_the_unmasked_upsample(s, levels):
    bits = 8 if levels == 255 else 16
    recs, rows = T.case(s, levels, kind="none")
    pool, offsets = T.pack(recs, bits)
    descs = T.descs_of(rows, offsets)
    P = T.CROPS[s]
    x, y, t, branch = T.synthesize(pool, descs, s, P, bits, levels, with_branch=True)
    assert not branch.any() and x.shape == y.shape == t.shape == (15, 1, P, P) and x.dtype == np.float32
    lv, lut = M.tables(bits, levels)
    for b, (i, H, W, y0, x0, op) in enumerate(rows):
        depth, guide, lr = recs[i]
        full = M.quantize(U.bicubic_upsample(lut[lr.astype(np.int64)][None, None], s), lv, lut)[0, 0]
        assert np.array_equal(x[b, 0].view(np.uint32), R.d4(full[y0:y0 + P, x0:x0 + P], op).view(np.uint32)), b
        assert np.array_equal(t[b, 0], lut[R.d4(depth[y0:y0 + P, x0:x0 + P], op).astype(np.int64)])
        assert np.array_equal(y[b, 0], R.lut()[R.d4(guide[y0:y0 + P, x0:x0 + P], op)])


@pytest.mark.parametrize("s", SCALES)
def test_the_standard_windows_reach_every_branch(s):
    """The GPU test's own condition, on the CPU: at least 10 % of the outputs in each branch of the rule."""
    recs, rows = T.case(s, 255)
    pool, offsets = T.pack(recs, 8)
    branch = T.synthesize(pool, T.descs_of(rows, offsets), s, T.CROPS[s], 8, with_branch=True)[3]
    share = np.bincount(branch.reshape(-1), minlength=3) / branch.size
    print(f"x{s}: branch shares {share}")
    assert (share >= 0.10).all(), share


# ---- TrainSet(lr_dir=...) -------------------------------------------------------------------------------------------------------

_write = T.write_set


@pytest.mark.parametrize("bits,levels", [(8, 255), (16, 65535), (16, 4096)])
def test_trainset_records_byte_for_byte(tmp_path, bits, levels):
    recs, _ = T.case(4, levels, shapes=((9, 13), (5, 7), (5, 7)))
    dd, cd, ld = _write(str(tmp_path), recs, bits, extra=(2, 0, 1, 3))       # larger planes are cropped top-left
    ts = train.TrainSet(dd, cd, "cpu", crop=16, depth_bits=bits, depth_max=levels, lr_dir=ld, scale=4)
    want, offsets = T.pack(recs, bits)
    assert ts.pool.dtype == torch.uint8 and np.array_equal(ts.pool.numpy(), want)
    assert ts.offsets.tolist() == offsets and ts.sizes.tolist() == [[36, 52], [20, 28], [20, 28]]
    assert (ts.has_lr, ts.lr_scale, ts.has_label, len(ts)) == (True, 4, False, 3)
    for off, (H, W), (depth, guide, lr) in zip(offsets, ts.sizes.tolist(), recs):
        got = T.planes(ts.pool.numpy(), off, H, W, 4, bits)
        assert all(np.array_equal(g, w) for g, w in zip(got, (depth, guide, lr)))
    # the target is the depth plane at the record's start: the integral images count ITS valid pixels
    ii = ts.valid_integrals()
    for off, (depth, _, _) in zip(offsets, recs):
        assert int(ii[off][-1, -1]) == int((depth != 0).sum())
    plain = train.TrainSet(dd, cd, "cpu", depth_bits=bits, depth_max=levels)
    assert (plain.has_lr, plain.lr_scale) == (False, None)


def test_trainset_refusals(tmp_path):
    recs, _ = T.case(4, 255, shapes=((9, 13), (5, 7)))
    dd, cd, ld = _write(str(tmp_path / "a"), recs, 8)
    for bad in (None, 2, 5, 32):
        with pytest.raises(ValueError, match="lr_dir needs scale"):
            train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=bad)
    with pytest.raises(ValueError, match="lr_dir and label_dir exclude each other"):
        train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4, label_dir=dd)
    with pytest.raises(ValueError, match="smaller than the 32x32 crop"):
        train.TrainSet(dd, cd, "cpu", crop=32, lr_dir=ld, scale=4)
    os.remove(os.path.join(ld, "01.png"))
    with pytest.raises(ValueError, match="01.png has no namesake in"):
        train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4)
    # the bit depth follows the set's, both ways, and a code above depth_max is refused: each names the LR file
    recs16, _ = T.case(4, 4096, shapes=((5, 7),))
    dd16, cd16, ld16 = _write(str(tmp_path / "b"), recs16, 16)
    with pytest.raises(ValueError, match=r"lr.00\.png: an 8-bit image in a 16-bit data set"):
        train.TrainSet(dd16, cd16, "cpu", depth_bits=16, depth_max=4096, lr_dir=os.path.join(str(tmp_path / "a"), "lr"), scale=4)
    with pytest.raises(ValueError, match=r"lr.00\.png: a 16-bit image"):
        train.TrainSet(dd, cd, "cpu", lr_dir=ld16, scale=4)
    hot = recs16[0][2].copy()
    hot[2, 3] = 4097
    io.write_depth16(os.path.join(ld16, "00.png"), hot)
    with pytest.raises(ValueError, match=r"lr.00\.png: code 4097 lies above depth_max 4096"):
        train.TrainSet(dd16, cd16, "cpu", depth_bits=16, depth_max=4096, lr_dir=ld16, scale=4)
    # a depth map or a guidance smaller than the LR file gives at the scale: refused by the file's name
    dd2, cd2, ld2 = _write(str(tmp_path / "c"), recs[:1], 8)
    with pytest.raises(ValueError, match=r"depth.00\.png: 36x52, smaller than the 72x104 that .*lr.00\.png gives at x8"):
        train.TrainSet(dd2, cd2, "cpu", lr_dir=ld2, scale=8)
    io.write_gray(os.path.join(cd2, "00.png"), recs[0][1][:, :51])
    with pytest.raises(ValueError, match=r"color.00\.png: 36x51, smaller than the 36x52"):
        train.TrainSet(dd2, cd2, "cpu", lr_dir=ld2, scale=4)


def test_synthesize_refusals(tmp_path):
    recs, rows = T.case(4, 255, shapes=((9, 13),))
    dd, cd, ld = _write(str(tmp_path), recs, 8)
    ts = train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4)
    descs = T.descs_of(rows, ts.offsets.tolist())
    with pytest.raises(ValueError, match="scale 8 with a TrainSet of x4"):
        train.synthesize(ts, descs, 8, 32)
    with pytest.raises(ValueError, match="degrade_holes and return_lr do not go"):
        train.synthesize(ts, descs, 4, 16, degrade_holes=True)
    with pytest.raises(ValueError, match="degrade_holes and return_lr do not go"):
        train.synthesize(ts, descs, 4, 16, return_lr=True)
    for crop in (12, 18):                                            # the existing rule on the crop holds here too
        with pytest.raises(ValueError, match="multiple of the scale 4 and at least 4 \\* scale"):
            train.synthesize(ts, descs, 4, crop)


# ---- host-side refusals of the entry point (decided before any launch) ----------------------------------------------------------

def _desc(n=1, crop=16, **f):
    d = L.CropDesc()
    d.n, d.crop = n, crop
    for b in range(max(min(n, L.TRAIN_MAX_BATCH), 0)):
        s = d.s[b]
        s.offset, s.height, s.width, s.y0, s.x0, s.op = 0, 36, 52, 0, 0, 0
        for k, v in f.items():
            setattr(s, k, v)
    return d


def test_entry_point_refusals_without_gpu():
    lib = L.load()
    p = C.c_void_p(4096)                                            # stands for every buffer: nothing is launched
    err = lambda: lib.codon_last_error_string()                     # noqa: E731
    rec8, rec16 = 2 * 36 * 52 + 9 * 13, 3 * 36 * 52 + 2 * 9 * 13

    def call(d=None, pool=p, nbytes=rec8, s=4, bits=8, lut=p, dm=255, lut8=p, wt=p, x=p, g=p, t=p):
        d = _desc() if d is None else d
        return lib.codon_train_crops_lr(C.byref(d) if d != "null" else None, pool, nbytes, s, bits, lut, dm, lut8, wt, x, g, t, None)

    for k in ("pool", "lut", "lut8", "wt", "x", "g", "t"):
        assert call(**{k: None}) == -1 and b"train_crops_lr: null pointer" in err(), k
    assert call(d="null") == -1 and b"null pointer" in err()
    assert call(d=_desc(n=0)) == -1 and b"batch 0" in err()
    assert call(d=_desc(n=L.TRAIN_MAX_BATCH + 1)) == -1 and b"batch 65" in err()
    for s in (0, 2, 3, 12, 32):
        assert call(s=s) == -2 and b"train_crops_lr: scale" in err(), s
    assert call(bits=12) == -1 and b"code_bits 12" in err()
    assert call(dm=256) == -1 and call(dm=254) == -1 and b"depth_max" in err()
    assert call(bits=16, dm=0, nbytes=rec16) == -1 and call(bits=16, dm=65536, nbytes=rec16) == -1 and b"depth_max" in err()
    assert call(d=_desc(crop=0)) == -1 and call(d=_desc(crop=2052)) == -1 and b"crop" in err()
    # H and W multiples of the scale
    assert call(d=_desc(height=37)) == -1 and b"no multiple of the scale 4" in err()
    assert call(d=_desc(width=50)) == -1 and b"no multiple of the scale 4" in err()
    assert call(s=8) == -1 and b"no multiple of the scale 8" in err()           # 36 x 52 at x8
    # the window inside the image
    for bad in (dict(y0=21), dict(x0=37), dict(y0=-1), dict(x0=-1), dict(op=8), dict(op=-1), dict(height=12, width=12)):
        assert call(d=_desc(**bad)) == -1 and b"outside the image" in err(), bad
    # the whole record inside the pool: the LR plane counts
    assert call(nbytes=rec8 - 1) == -1 and b"runs past the" in err()
    assert call(nbytes=2 * 36 * 52) == -1 and call(d=_desc(offset=1)) == -1 and b"runs past the" in err()
    assert call(d=_desc(offset=-1)) == -1 and b"negative" in err()
    assert call(bits=16, dm=4096, nbytes=rec16 - 1) == -1 and b"runs past the" in err()
    far = dict(height=36, width=44, offset=2)                       # another size, and not the pool's first record
    for bits, dm, rec in ((8, 255, 2 * 36 * 44 + 9 * 11), (16, 4096, 3 * 36 * 44 + 2 * 9 * 11)):
        assert call(bits=bits, dm=dm, nbytes=2 + rec - 1, d=_desc(**far)) == -1 and b"runs past the" in err(), bits
    # 16 bits: an even offset and a 2-byte-aligned pool
    assert call(bits=16, dm=4096, nbytes=rec16 + 2, d=_desc(offset=1)) == -1 and b"odd" in err()
    assert call(bits=16, dm=4096, nbytes=rec16, pool=C.c_void_p(4097)) == -1 and b"not 2-byte aligned" in err()
    # only the LAST sample bad: every sample is checked
    d = _desc(n=3)
    d.s[2].x0 = 37
    assert call(d=d) == -1 and b"sample 2" in err()


# ---- the command line and the resume key ----------------------------------------------------------------------------------------

def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_train_cli_option_and_refusals(capsys):
    a = train.parse_args(_argv())
    assert a.train_lr_depth is None and "train_lr_depth" not in train.run_args(a)
    a = train.parse_args(_argv("--train-lr-depth", "l"))
    assert a.train_lr_depth == "l" and train.run_args(a)["train_lr_depth"] is True
    a = train.parse_args(_argv("--train-lr-depth", "l", "--depth-bits", "16", "--depth-max", "4096", "--mask-holes", "--min-valid",
                               "0.5", "--val-lr-depth", "v", "--val-color", "vc"))
    r = train.run_args(a)
    assert (r["train_lr_depth"], r["depth_bits"], r["depth_max"], r["mask_holes"], r["min_valid"]) == (True, 16, 4096, True, 0.5)
    with pytest.raises(SystemExit) as e:
        train.parse_args(_argv("--train-lr-depth", "l", "--train-label", "t"))
    assert e.value.code == 2 and "--train-lr-depth and --train-label exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        train.parse_args(_argv("--train-lr-depth", "l", "--degrade-holes"))
    assert e.value.code == 2 and "--train-lr-depth and --degrade-holes exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit):                                  # --train-depth stays required: it is the target
        train.parse_args(["--scale", "4", "--train-lr-depth", "l", "--train-color", "c"])
    assert "--train-depth" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(_argv("--train-lr-depth", "l", "--crop", "12"))
    assert "--crop 12 must be a multiple" in capsys.readouterr().err


def test_resume_key_three_ways(tmp_path):
    assert train.LR_DEFAULTS == {"train_lr_depth": False}
    plain = train.run_args(train.parse_args(_argv()))
    paired = train.run_args(train.parse_args(_argv("--train-lr-depth", "l")))
    assert "train_lr_depth" not in plain                            # an older checkpoint, and one of a run without the option
    ck = {"epoch": 2, "model": {}, "optimizer": {}, "rng": np.random.default_rng(0).bit_generator.state, "args": plain}
    p = str(tmp_path / "ck.pth")
    torch.save(ck, p)
    assert train.load_resume(p, plain)["epoch"] == 2
    with pytest.raises(ValueError, match="other arguments: train_lr_depth False != True"):
        train.load_resume(p, paired)
    torch.save(dict(ck, args=paired), p)
    got = train.load_resume(p, paired)
    assert got["epoch"] == 2 and got["args"]["train_lr_depth"] is True
    with pytest.raises(ValueError, match="train_lr_depth True != False"):
        train.load_resume(p, plain)
