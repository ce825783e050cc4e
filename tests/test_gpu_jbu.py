"""The classical baselines on the MI355X: joint bilateral upsampling against the numpy restatement tests/jbu_ref.py
(pinned on the CPU by tests/test_jbu_cpu.py), the bicubic baseline against the integer the input restatement looks up, and the
baselines in the network's place in infer.  The bar is EQUAL BITS throughout, no tolerance anywhere.
Shapes are the fillers', each at guided_fill_ref.SHAPE_SCALE's scale, the smallest at which each part can go wrong: one pixel (a
footprint almost wholly outside the plane), odd sizes (28 wide at x4: a partial run of 12 pixels), a batch, exactly one tile of
cells for the G_0 launch, one cell past it on both axes at x16 (1040 x 1072: tile edges on both axes, a last partial tile of
pixels), and 70 x 200 at x4 (800 wide: seven tiles across, the last a quarter wide)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops
from codon_amd.upsample import (bicubic_upsample_codes, fill_holes_guided, joint_bilateral_upsample, spatial_table, stretch_codes,
                                unstretch_codes)
from tests import fill_ref as F
from tests import guided_fill_ref as R
from tests import jbu_ref as J
from tests import resample_masked_ref as M
from tests import stretch_ref as T
from tests.test_jbu_cpu import jbu_caller, jbu_refusals

pytestmark = pytest.mark.gpu

quiet = lambda s: None                                               # noqa: E731
ids = lambda s: "x".join(map(str, s))                                # noqa: E731


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy() if t.dtype != torch.bfloat16 else t.view(torch.int16).cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _in_place(g):
    """(the guide inside a larger tensor, that tensor): rows W + 3 bytes apart and images a number of bytes apart that is no
    multiple of 16, so that the runs of most rows start off a 16-byte boundary: the byte path, beside the 16-byte one in the same
    launch where a row happens to be aligned"""
    B, H, W = g.shape
    rows = next(r for r in range(H + 1, H + 17) if (r * (W + 3)) % 16)
    big = np.full((B, rows, W + 3), 201, dtype=np.uint8)
    big[:, :H, :W] = g
    whole = torch.from_numpy(big).cuda()
    view = whole[:, :H, :W]
    assert view.stride(1) == W + 3 and view.stride(0) % 16 != 0 and not view.is_contiguous()
    return view, whole


@pytest.mark.parametrize("shape", F.SHAPES, ids=ids)
def test_equals_the_restatement(shape):
    """jbu_ref.cases: every pattern, format, kind of guidance and sigma_s, each with a dense guide (16 bytes per lane where a run
    is whole) and with the guide read in place from a larger tensor (bytes); no argument is modified."""
    s = R.SHAPE_SCALE[shape]
    guides = {}
    for kind in R.GUIDES:
        g = R.guide_case(shape, s, kind)
        guides[kind] = (torch.from_numpy(g.copy()).cuda(), *_in_place(g))
    for name, top, pattern, kind, sigma_s, _ in J.cases(shape):
        want = J.want(shape, pattern, top, s, kind, 10.0, sigma_s)
        src = _codes_dev(F.case(shape, pattern, top))
        before = src.clone()
        dense, view, whole = guides[kind]
        keep = whole.clone()
        dm = None if top == 255 else top
        for how, gd in (("dense", dense), ("in place", view)):
            got = joint_bilateral_upsample(src, gd, s, sigma_s, depth_max=dm)
            assert got.shape == want.shape and got.dtype == src.dtype and got.is_contiguous()
            bad = np.argwhere(_bits(got) != want)
            assert bad.size == 0, f"{shape} {name} {pattern} {kind} {sigma_s} {how}: {len(bad)} values differ, first at {bad[:3].tolist()}"
        assert torch.equal(src, before) and torch.equal(whole, keep) and torch.equal(dense, view), "an argument was modified"
        if pattern == "all":
            assert not got.any()
        if pattern == "none":
            assert (got != 0).all()


def test_plane_forms_tables_and_streams():
    """(h, w) planes with (H, W) guides, uint16 tensors, sigma_r and the tests' own table, and two streams with a workspace each."""
    shape, s = (3, 9, 13), 8
    codes, g = F.case(shape, "levels", 65535), R.guide_case(shape, s, "scene")
    want = J.want(shape, "levels", 65535, s, "scene", 10.0, 1.0)
    dev, gd = _codes_dev(codes), torch.from_numpy(g.copy()).cuda()
    one = joint_bilateral_upsample(dev[1], gd[1], s)
    assert one.shape == (72, 104) and one.dtype == torch.int16 and np.array_equal(_bits(one), want[1])
    u16 = joint_bilateral_upsample(dev.view(torch.uint16), gd, s)
    assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want)
    assert np.array_equal(_bits(joint_bilateral_upsample(dev, gd, s, 0.5, 3.0)), J.want(shape, "levels", 65535, s, "scene", 3.0, 0.5))
    c37 = torch.from_numpy(R.table_of("c37").view(np.int16).copy()).cuda()
    flat = joint_bilateral_upsample(dev, gd, s, _table=c37)
    assert np.array_equal(_bits(flat), J.want(shape, "levels", 65535, s, "scene", "c37", 1.0))
    assert torch.equal(joint_bilateral_upsample(dev, torch.full_like(gd, 113), s), flat)      # a constant guide: the same bits
    st = spatial_table(s, 1.0, dev.device)
    assert st.shape == (s, 4) and st.dtype == torch.int16 and np.array_equal(_bits(st), J.spatial_table(s, 1.0))
    torch.cuda.synchronize()
    outs = []
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            outs.append(joint_bilateral_upsample(dev, gd, s))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and np.array_equal(_bits(outs[0]), want)
    with pytest.raises(ValueError, match="joint_bilateral_upsample: a 72x103 guide, smaller than the 72x104"):
        joint_bilateral_upsample(dev, torch.zeros(3, 72, 103, dtype=torch.uint8, device="cuda"), s)
    with pytest.raises(ValueError, match="2 guidance images for 3 maps"):
        joint_bilateral_upsample(dev, torch.zeros(2, 72, 104, dtype=torch.uint8, device="cuda"), s)
    with pytest.raises(ValueError, match="unit stride along a row"):
        joint_bilateral_upsample(dev, torch.zeros(3, 72, 208, dtype=torch.uint8, device="cuda")[:, :, ::2], s)
    with pytest.raises(RuntimeError, match="expects a uint8 guide"):
        joint_bilateral_upsample(dev, torch.zeros(3, 72, 104, device="cuda"), s)
    with pytest.raises(ValueError, match="joint_bilateral_upsample: sigma_s 0"):
        joint_bilateral_upsample(dev, gd, s, 0)
    with pytest.raises(ValueError, match="joint_bilateral_upsample: scale 2 "):
        joint_bilateral_upsample(dev, gd, 2)


@pytest.mark.parametrize("s", [8, 16])
def test_tiles_at_the_other_scales(s):
    """The widest plane at x8 and x16 (test_equals_the_restatement runs it at x4): the other two window widths over many tiles,
    with a last partial tile (1600 and 3200 wide: half a tile)."""
    shape = (1, 70, 200)
    gd = torch.from_numpy(R.guide_case(shape, s, "random").copy()).cuda()
    got = joint_bilateral_upsample(_codes_dev(F.case(shape, "levels", 65535)), gd, s)
    assert np.array_equal(_bits(got), J.want(shape, "levels", 65535, s, "random", 10.0, 1.0))


def test_refusals_leave_out_untouched():
    lib = L.load()
    B, h, w, s = 1, 5, 7, 4
    src = _codes_dev(F.case((B, h, w), "cross", 65535))
    gd = torch.from_numpy(R.guide_case((B, h, w), s, "random").copy()).cuda()
    gd2 = torch.cat([gd, gd])                                        # (the refusal of a short image stride names two images)
    tab = torch.from_numpy(R.table_of(10.0).view(np.int16).copy()).cuda()
    stab = spatial_table(s, 1.0, src.device)
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((2, h * s, w * s), -21555, dtype=torch.int16, device="cuda")
    keep_src = src.clone()
    call = jbu_caller(lib, src.data_ptr(), gd2.data_ptr(), tab.data_ptr(), stab.data_ptr(), out.data_ptr(), ws.data_ptr(),
                      ops._stream(torch.device("cuda:0")))
    jbu_refusals(lib, call)
    assert "unaligned" in call(src=src.data_ptr() + 1)[1] and "unaligned" in call(out=out.data_ptr() + 8)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and torch.equal(src, keep_src)
    assert call()[0] == 0                                            # and the good call they all differ from goes through
    assert np.array_equal(_bits(out[0]), J.want((B, h, w), "cross", 65535, s, "random", 10.0, 1.0)[0]) and (out[1] == -21555).all()


# ---- the bicubic baseline ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", F.SHAPES, ids=ids)
def test_bicubic_codes_and_the_input_beside_them(shape):
    """bicubic_upsample_codes is the integer the input restatement looks up, rint(clamp(up) levels), on the same planes; the
    float input built beside it from the same codes keeps its bits (the kernel is one text with two ways out)."""
    s = R.SHAPE_SCALE[shape]
    for name, top, pattern, *_ in J.cases(shape):
        codes = F.case(shape, pattern, top)
        src = _codes_dev(codes)
        before = src.clone()
        dm = None if top == 255 else top
        want = J.bicubic_codes(codes, s, top)
        got = bicubic_upsample_codes(src, s, dm)
        assert got.shape == want.shape and got.dtype == src.dtype
        bad = np.argwhere(_bits(got) != want)
        assert bad.size == 0, f"{shape} {name} {pattern}: {len(bad)} codes differ, first at {bad[:3].tolist()}"
        levels, lut = M.tables(8 if top == 255 else 16, top)
        x = infer.codes_to_input(src, s, torch.float32, dm)
        assert np.array_equal(_bits(x)[:, 0], np.asarray(lut, dtype=np.float32)[want.astype(np.int64)].view(np.uint32))
        assert torch.equal(src, before)
    one = bicubic_upsample_codes(src[0], s, dm)
    assert one.shape == want.shape[1:] and np.array_equal(_bits(one), want[0])
    with pytest.raises(ValueError, match="bicubic_upsample_codes: scale 3 "):
        bicubic_upsample_codes(src, 3, dm)


def test_the_input_restatement_itself_is_unchanged():
    """codes_to_input against resample_masked_ref.codes_to_input itself, in the three dtypes, on the shapes that restatement
    takes no seconds for"""
    for shape in F.SHAPES[:3]:
        s = R.SHAPE_SCALE[shape]
        for top in (255, 10000):
            codes = F.case(shape, "levels", top)
            levels, lut = M.tables(8 if top == 255 else 16, top)
            for tdt, name in ((torch.float32, "f32"), (torch.float16, "f16"), (torch.bfloat16, "bf16")):
                got = infer.codes_to_input(_codes_dev(codes), s, tdt, None if top == 255 else top)
                ref = M.codes_to_input(codes, s, levels, lut, name)
                assert np.array_equal(_bits(got), ref.view(_bits(got).dtype)), (shape, top, name)


# ---- the baselines in the network's place --------------------------------------------------------------------------------------------

def _write_files(root, bits, depth_max, s=4):
    """lr/, color/ and label/ with three occlusion scenes of 24 x 32 with the scene's holes: (dirs, [(holed codes, guide)])"""
    dirs = [os.path.join(root, n) for n in ("lr", "color", "label")]
    for d in dirs:
        os.makedirs(d)
    top = 255 if bits == 8 else depth_max
    write = io.write_gray if bits == 8 else io.write_depth16
    cases = []
    for i in range(3):
        _, holed, guide, truth, _ = J.hr_scene(24, 32, s, top, seed=3 + i)
        write(os.path.join(dirs[0], f"{i:02d}.png"), holed)
        io.write_gray(os.path.join(dirs[1], f"{i:02d}.png"), guide)
        write(os.path.join(dirs[2], f"{i:02d}.png"), truth)
        cases.append((holed, guide))
    return dirs, cases


def _composition(baseline, holed, guide, s, top, sigma_s=1.0):
    """fill -> stretch -> the baseline -> unstretch, in the numpy restatements"""
    filled = R.fill_plane(holed, guide, s, R.range_table(10.0))
    lo, hi = T.code_range(filled)
    st = T.stretch(filled, lo, hi, top)
    up = (J.upsample_plane(st, guide, s, R.range_table(10.0), J.spatial_table(s, sigma_s)) if baseline == "jbu" else
          J.bicubic_codes(st[None], s, top)[0])
    return T.unstretch(up, lo, hi, top)


def _read(path, bits, depth_max):
    return io.read_depth_plane(path, bits, depth_max)


@pytest.mark.parametrize("baseline", ["jbu", "bicubic"])
def test_infer_main_with_a_baseline(tmp_path, capsys, baseline):
    """--baseline B --fill-holes --fill-guided --normalize --report: pipelined and --serial print the same lines and write the
    same bytes, no model is built (no warning about weights), and the PNGs are the composition of the numpy restatements."""
    s = 4
    (lrd, cd, ld), cases = _write_files(str(tmp_path), 8, 255, s)
    outs = {}
    for mode in ("pipe", "serial"):
        od = tmp_path / f"out_{mode}"
        capsys.readouterr()
        rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", ld, "--out", str(od), "--baseline", baseline,
                         "--fill-holes", "--fill-guided", "--normalize", "--report", "--bad-thresholds", "1,4", "--edge-threshold", "20",
                         "--dtype", "bf16"] + (["--serial"] if mode == "serial" else []))
        assert rc == 0
        outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in sorted(os.listdir(od))})
    assert outs["pipe"] == outs["serial"] and len(outs["pipe"][1]) == 3
    text = outs["pipe"][0]
    assert "WARNING" not in text and "loaded epoch" not in text
    lines = text.strip().splitlines()
    assert len(lines) == 6 and lines[0].startswith("00.png ") and "mad=" in lines[0] and lines[3] == "3" and lines[5].startswith("mean ")
    for i, (holed, guide) in enumerate(cases):
        got = _read(str(tmp_path / "out_pipe" / f"{i:02d}.png"), 8, 255)
        want = _composition(baseline, holed, guide, s, 255)
        assert got.shape == (96, 128) and np.array_equal(got, want), (baseline, i, int((got != want).sum()))


def test_run_loop_with_a_baseline(tmp_path):
    """run_loop(baseline=): both loops give the composition of the device functions and of the numpy restatements, with and
    without the preparation; the sigmas reach the upsampler; 16-bit files at depth_max 10000 run once."""
    s = 4
    dev = torch.device("cuda:0")
    (lrd, cd, ld), cases = _write_files(str(tmp_path / "8"), 8, 255, s)
    kw = dict(emit=quiet, lr_depth=lrd, scale=s)
    rows = {}
    for pipelined in (True, False):
        lines = []
        od = tmp_path / f"o{pipelined}"
        os.makedirs(od)
        r = infer.run_loop(None, dev, torch.float32, None, cd, ld, str(od), pipelined=pipelined, baseline="jbu", jbu_sigma_s=0.5,
                           **dict(kw, emit=lines.append))
        assert r["n"] == 3 and r["rmse_mean"] is not None
        rows[pipelined] = (lines, r["rmse_mean"], r["ssim_mean"], {n: open(od / n, "rb").read() for n in sorted(os.listdir(od))})
    assert rows[True] == rows[False]
    for i, (holed, guide) in enumerate(cases):                      # no preparation: the holes' band stays where no tap is valid
        got = _read(str(tmp_path / "oTrue" / f"{i:02d}.png"), 8, 255)
        want = J.upsample_plane(holed, guide, s, R.range_table(10.0), J.spatial_table(s, 0.5))
        assert np.array_equal(got, want)
        gd = torch.from_numpy(guide.copy()).cuda()
        assert np.array_equal(_bits(joint_bilateral_upsample(_codes_dev(holed), gd, s, 0.5)), want)
        st, lo_hi = stretch_codes(fill_holes_guided(_codes_dev(holed), gd, s))
        assert np.array_equal(_bits(unstretch_codes(joint_bilateral_upsample(st, gd, s), lo_hi)), _composition("jbu", holed, guide, s, 255))
    od = tmp_path / "sigma_r"
    os.makedirs(od)
    infer.run_loop(None, dev, torch.float32, None, cd, None, str(od), baseline="jbu", jbu_sigma_s=0.5, jbu_sigma_r=3.0, **kw)
    assert any(open(od / n, "rb").read() != rows[True][3][n] for n in rows[True][3])
    (lrd, cd, ld), cases = _write_files(str(tmp_path / "16"), 16, 10000, s)
    for baseline in ("jbu", "bicubic"):
        od = tmp_path / f"deep_{baseline}"
        os.makedirs(od)
        r = infer.run_loop(None, dev, torch.float32, None, cd, ld, str(od), baseline=baseline, depth_bits=16, depth_max=10000,
                           fill_holes=True, fill_guided=True, normalize=True, report={"thresholds": (10,), "edge_threshold": 500},
                           emit=quiet, lr_depth=lrd, scale=s)
        assert r["n"] == 3 and len(r["reports"]) == 3
        for i, (holed, guide) in enumerate(cases):
            got = _read(str(od / f"{i:02d}.png"), 16, 10000)
            assert got.dtype == np.uint16 and np.array_equal(got, _composition(baseline, holed, guide, s, 10000)), (baseline, i)


def test_infer_main_16_bit_once(tmp_path, capsys):
    (lrd, cd, ld), cases = _write_files(str(tmp_path), 16, 10000)
    od = tmp_path / "out"
    rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", ld, "--out", str(od), "--baseline", "jbu",
                     "--jbu-sigma-s", "0.5", "--jbu-sigma-r", "8", "--depth-bits", "16", "--depth-max", "10000", "--report"])
    assert rc == 0 and "WARNING" not in capsys.readouterr().out
    holed, guide = cases[1]
    want = J.upsample_plane(holed, guide, 4, R.range_table(8.0), J.spatial_table(4, 0.5))
    assert np.array_equal(_read(str(od / "01.png"), 16, 10000), want)
