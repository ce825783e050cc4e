"""The hole-aware resampling without a GPU: the numpy restatement against the existing restatements, its
branch map, the host-side refusals of the three entry points and of the command lines, and the resume key."""
import ctypes as C

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, train
from oracle import upsample_oracle as U
from tests import resample_masked_ref as M
from tests import train_data_ref as R

SCALES = (4, 8, 16)


@pytest.mark.parametrize("s", SCALES)
def test_hole_free_planes_give_the_existing_bits(s):
    lr = M.plane(2, 5, 7, "none", seed=s)
    out, valid = M.upsample_masked(lr, s)
    assert valid.all() and np.array_equal(out.view(np.uint32), U.bicubic_upsample(lr, s).view(np.uint32))
    for levels in (255, 10000):
        lv, lut = M.tables(8 if levels == 255 else 16, levels)
        hr = M.plane(2, 4 * s, 4 * s, "none", seed=s + 1)
        got = M.downsample_masked(hr, s, lv, lut)
        want = M.snap(R.downsample(hr, s), lv, lut)                 # equality holds after the >= 1 snap
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and (got != 0).all()


@pytest.mark.parametrize("s", SCALES)
def test_all_holes_and_a_single_valid_pixel(s):
    out, valid = M.upsample_masked(M.plane(1, 5, 7, "all"), s)
    assert not valid.any() and not out.any() and not np.signbit(out).any()
    assert not M.downsample_masked(M.plane(1, 4 * s, 4 * s, "all"), s, 255, R.lut()).any()
    out, valid = M.upsample_masked(M.plane(1, 5, 7, "one"), s)
    assert np.isfinite(out).all() and valid.any() and not out[~valid].any()
    lr = M.downsample_masked(M.plane(1, 4 * s, 4 * s, "one"), s, 255, R.lut())
    assert np.isfinite(lr).all()


@pytest.mark.parametrize("s", SCALES)
def test_the_pattern_reaches_every_branch(s):
    """6 % isolated holes plus one 4 x 5 blob on a 9 x 13 plane: at least 5 % of the outputs in EACH of the three branches,
    so no branch goes untested where the GPU tests use this pattern."""
    _, valid, branch = M.upsample_masked(M.plane(1, 9, 13, "pattern"), s, with_branch=True)
    share = np.bincount(branch.reshape(-1), minlength=3) / branch.size
    print(f"x{s}: branch shares {share}")
    assert (share >= 0.05).all(), share
    assert np.array_equal(valid, branch != 2)


def test_down_snap_never_gives_code_zero():
    lut = R.lut()
    hr = M.plane(1, 32, 32, "pattern", seed=3)
    hr[hr != 0] = np.float32(1e-4)                                  # rounds to code 0 unsnapped
    lr, branch = M.downsample_masked(hr, 4, 255, lut, with_branch=True)
    assert ((lr == 0) == (branch == 2)).all() and (lr[branch != 2] == lut[1]).all()


def test_fused_restatement_is_the_composition():
    codes = np.random.default_rng(5).integers(0, 256, size=(2, 5, 7))
    v = R.lut()[codes][:, None]
    up, _ = M.upsample_masked(v, 4)
    assert np.array_equal(M.codes_to_input(codes, 4, 255, R.lut()), R.quantize(up))


# ---- host-side refusals of the entry points (decided before any launch) -------------------------------------------------------

def test_entry_point_refusals_without_gpu():
    lib = L.load()
    p = C.c_void_p(4096)                                            # stands for every buffer: nothing is launched
    err = lambda: lib.codon_last_error_string()                     # noqa: E731
    up = lambda B=1, h=5, w=7, s=4, lr=p, wt=p, out=p: lib.codon_bicubic_upsample_masked(B, h, w, s, lr, wt, out, None, None)  # noqa: E731
    assert up(lr=None) == -1 and b"null pointer" in err()
    assert up(out=None) == -1 and up(wt=None) == -1
    assert up(s=3) == -2 and b"scale 3" in err()
    assert up(B=0) == -1 and up(h=0) == -1 and up(w=70000) == -1 and b"bad shape" in err()
    dn = lambda B=1, P=32, s=4, hr=p, wt=p, lut=p, lv=255, out=p: lib.codon_bicubic_downsample_masked(B, P, s, hr, wt, lut, lv, out, None)  # noqa: E731
    assert dn(hr=None) == -1 and dn(wt=None) == -1 and dn(lut=None) == -1 and dn(out=None) == -1
    assert dn(s=2) == -2
    for bad in (dict(P=12), dict(P=34), dict(P=1028), dict(P=2048), dict(B=0), dict(B=65536), dict(s=16, P=32)):
        assert dn(**bad) == -1 and b"bicubic_downsample_masked: batch" in err(), bad
    assert dn(lv=0) == -1 and dn(lv=65536) == -1 and b"levels" in err()
    cv = lambda B=1, h=5, w=7, s=4, c=p, bits=8, lut=p, dm=255, wt=p, out=p, dt=L.F16: lib.codon_lr_codes_to_input(  # noqa: E731
        B, h, w, s, c, bits, lut, dm, wt, out, dt, None)
    assert cv(c=None) == -1 and cv(lut=None) == -1 and cv(wt=None) == -1 and cv(out=None) == -1
    assert cv(s=5) == -2 and cv(dt=7) == -2
    assert cv(bits=12) == -1 and b"code_bits" in err()
    assert cv(dm=256) == -1 and cv(bits=16, dm=0) == -1 and cv(bits=16, dm=65536) == -1 and b"depth_max" in err()
    assert cv(B=0) == -1 and cv(h=0) == -1 and cv(w=-1) == -1
    assert cv(out=C.c_void_p(4104)) == -1 and b"aligned" in err()
    assert cv(bits=16, dm=4096, c=C.c_void_p(4097)) == -1 and b"aligned" in err()


# ---- the command lines ----------------------------------------------------------------------------------------------------------

def test_infer_refuses_both_or_neither_depth_source(capsys):
    with pytest.raises(SystemExit) as e:
        infer.main(["--input-depth", "a", "--lr-depth", "b", "--input-color", "c"])
    assert e.value.code == 2 and "exactly one of --input-depth and --lr-depth" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        infer.main(["--input-color", "c"])
    assert e.value.code == 2 and "exactly one of --input-depth and --lr-depth" in capsys.readouterr().err
    with pytest.raises(ValueError, match="exactly one"):
        infer.run_loop(None, None, torch.float32, "a", "c", lr_depth="b", scale=4)
    with pytest.raises(ValueError, match="needs scale"):
        infer.run_loop(None, None, torch.float32, None, "c", lr_depth="b")


def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_train_cli_options_and_refusals(capsys):
    a = train.parse_args(_argv())
    assert (a.degrade_holes, a.val_lr_depth) == (False, None) and "degrade_holes" not in train.run_args(a)
    a = train.parse_args(_argv("--degrade-holes"))                  # needs no other flag
    assert a.degrade_holes and train.run_args(a)["degrade_holes"] is True
    a = train.parse_args(_argv("--val-lr-depth", "v", "--val-color", "vc"))
    assert (a.val_lr_depth, a.val_depth) == ("v", None)
    with pytest.raises(SystemExit) as e:
        train.parse_args(_argv("--val-lr-depth", "v", "--val-depth", "w", "--val-color", "vc"))
    assert e.value.code == 2 and "--val-depth and --val-lr-depth exclude each other" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(_argv("--val-lr-depth", "v"))
    assert "--val-color go together" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(_argv("--degrade-holes", "--crop", "2048"))
    assert "--degrade-holes takes crops up to 1024" in capsys.readouterr().err


def test_resume_default_for_a_checkpoint_without_the_key(tmp_path):
    plain = train.run_args(train.parse_args(_argv()))
    holes = train.run_args(train.parse_args(_argv("--degrade-holes")))
    assert "degrade_holes" not in plain                              # an older checkpoint, and one of a run without the option
    ck = {"epoch": 2, "model": {}, "optimizer": {}, "rng": np.random.default_rng(0).bit_generator.state, "args": plain}
    p = str(tmp_path / "ck.pth")
    torch.save(ck, p)
    assert train.load_resume(p, plain)["epoch"] == 2
    with pytest.raises(ValueError, match="other arguments: degrade_holes False != True"):
        train.load_resume(p, holes)
    torch.save(dict(ck, args=holes), p)
    assert train.load_resume(p, holes)["epoch"] == 2
    with pytest.raises(ValueError, match="degrade_holes True != False"):
        train.load_resume(p, plain)
