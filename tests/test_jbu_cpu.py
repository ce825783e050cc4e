"""The joint bilateral upsampler's definition (tests/jbu_ref.py) on the CPU: what the definition promises, the edge
claim that makes it a baseline worth printing, and every refusal that needs no GPU -- of the C entries (validated on the host before
any HIP call), of spatial_table, and of the command line."""
import ctypes as C

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer
from codon_amd.upsample import JBU_SIGMA_S, spatial_table
from tests import fill_ref as F
from tests import guided_fill_ref as R
from tests import jbu_ref as J

SHAPES = sorted(R.SHAPE_SCALE.items())
ids = lambda v: "x".join(map(str, v[0])) + f"@{v[1]}"                                     # noqa: E731
T10 = R.range_table(10.0)


def _const(n, shape=(256,)):
    return np.full(shape, n, dtype=np.uint16)


def test_spatial_table_is_the_restatement_and_refuses():
    assert JBU_SIGMA_S == J.SIGMA_S == 1.0
    for s in J.SCALES:
        for sigma in (0.5, 1.0, 3.0):
            t = spatial_table(s, sigma)
            assert t.shape == (s, 4) and t.dtype == np.uint16 and not t.flags.writeable
            assert np.array_equal(t, J.spatial_table(s, sigma)) and t.min() >= 1 and t.max() <= 256
            assert np.array_equal(t, t[::-1, ::-1])                                      # phase s - 1 - ph mirrors the taps
        assert (spatial_table(s)[:, 1:3].max(axis=1) >= 226).all()                       # the nearer of the two inner taps: d <= 1 / 2
    assert spatial_table(4) is spatial_table(4, 1.0)                                     # cached
    for bad in (0, -1.0, float("inf"), float("nan"), "x", None):
        with pytest.raises(ValueError, match="spatial_table: sigma_s"):
            spatial_table(4, bad)
    with pytest.raises(ValueError, match="spatial_table: scale 2 "):
        spatial_table(2)


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_constant_table_and_constant_guide(case):
    """Under a constant range table the guide has no say, and a constant guide under any table gives the same bits."""
    shape, s = case
    S = J.spatial_table(s)
    small = shape in J.CROSSED                                                           # the larger planes: one pattern, fewer tables
    for pattern, top in ((("levels", 255), ("cross", 65535), ("border", 10000)) if small else (("levels", 10000),)):
        c = F.case(shape, pattern, top)
        outs = [J.upsample(c, R.guide_case(shape, s, kind), s, _const(n), S) for kind in ("random", "scene")
                for n in ((1, 37, 256) if small else (37,))]
        outs.append(J.upsample(c, R.guide_case(shape, s, "constant"), s, T10, S))
        outs.append(J.upsample(c, R.guide_case(shape, s, "constant"), s, R.range_table(3.0), S))
        assert all(np.array_equal(o, outs[0]) for o in outs[1:]), (pattern, top)
        assert not np.array_equal(J.upsample(c, R.guide_case(shape, s, "random"), s, T10, S), outs[0]) or shape == (1, 1, 1)


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_range_and_holes(case):
    """A non-zero output lies within [min, max] of its valid taps; the output is 0 exactly where the footprint holds no valid
    code; a dense map gives no zero."""
    shape, s = case
    for pattern in F.PATTERNS:
        for top in ((255, 10000) if shape in J.CROSSED else (10000,)):
            c = F.case(shape, pattern, top)
            out = J.upsample(c, R.guide_case(shape, s, "random"), s, T10, J.spatial_table(s, 0.5))
            assert out.dtype == c.dtype and out.shape == (shape[0], shape[1] * s, shape[2] * s)
            for p, o in zip(c, out):
                any_, lo, hi = J.footprint_valid(p, s)
                assert np.array_equal(o != 0, any_), (pattern, top)
                assert (o[any_] >= lo[any_]).all() and (o[any_] <= hi[any_]).all(), (pattern, top)
            if pattern == "none":
                assert out.min() >= 1
            if pattern == "all":
                assert not out.any()


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_the_numerator_bound_is_reached(case):
    """An all-top u16 plane comes back all top; with both tables at 256 an interior pixel reaches sum w = 2^20 and the stated
    numerator, which 64 bits hold and 32 do not."""
    shape, s = case
    c = np.full(shape[1:], 65535, dtype=np.uint16)
    g = R.guide_case(shape, s, "random")[0]
    out, top_num = J.upsample_plane(c, g, s, _const(256), _const(256, (s, 4)), with_sums=True)
    assert (out == 65535).all()
    if min(shape[1:]) >= 4:
        assert top_num == J.NUMERATOR_MAX == 2 * (1 << 20) * 65535 + (1 << 20) and top_num > 1 << 32
    out8, top8 = J.upsample_plane(np.full(shape[1:], 255, dtype=np.uint8), g, s, _const(256), _const(256, (s, 4)), with_sums=True)
    assert (out8 == 255).all() and top8 <= J.NUMERATOR_MAX_U8 < 1 << 30
    assert (J.upsample_plane(c, g, s, T10, J.spatial_table(s)) == 65535).all()


@pytest.mark.parametrize("case", SHAPES, ids=ids)
def test_u8_and_u16_agree(case):
    shape, s = case
    g = R.guide_case(shape, s, "scene")
    for pattern in ("levels", "one"):
        c8 = F.case(shape, pattern, 255)
        a = J.upsample(c8, g, s, T10, J.spatial_table(s))
        b = J.upsample(c8.astype(np.uint16), g, s, T10, J.spatial_table(s))
        assert a.dtype == np.uint8 and b.dtype == np.uint16 and np.array_equal(a, b)


@pytest.mark.parametrize("top", [255, 10000])
@pytest.mark.parametrize("s", J.SCALES)
def test_the_edge_claim(s, top):
    """On the high-resolution occlusion scene without holes the joint bilateral upsampler's mean absolute error in the edge region
    is at most a tenth of the bicubic's (measured 1/30 to 1/90), and in the flat region it is not above the bicubic's."""
    codes, _, guide, truth, near = J.hr_scene(24, 32, s, top)
    edge = J.edge_region(near, s)
    assert 0.02 < edge.mean() < 0.25 and (codes != 0).all()
    bic = J.bicubic_codes(codes[None], s, top)[0]
    for sigma_s in J.SIGMAS_S:
        out = J.upsample_plane(codes, guide, s, T10, J.spatial_table(s, sigma_s))
        je, be = J.mad(out, truth, edge), J.mad(bic, truth, edge)
        jf, bf = J.mad(out, truth, ~edge), J.mad(bic, truth, ~edge)
        print(f"x{s} top {top} sigma_s {sigma_s}: edge {je / top:.5f} vs {be / top:.5f}, flat {jf / top:.5f} vs {bf / top:.5f}")
        assert je <= be / 10 and jf <= bf


def test_bicubic_codes_is_the_input_restatement_in_codes():
    """jbu_ref.bicubic_codes, the yardstick of bicubic_upsample_codes, is rint(resample_masked_ref.codes_to_input(., "f32") levels)
    bit for bit -- on the shapes small enough for that restatement's count of invalid taps -- and truncating instead, as
    post-processing does, would lose codes."""
    from tests import resample_masked_ref as M
    lost = 0
    for shape, s in SHAPES:
        if shape[1] * shape[2] > 64 * 64:
            continue
        small = shape[1] * shape[2] < 64 * 64                                           # the tile-sized plane: one case
        for pattern in (F.PATTERNS if small else ("levels",)):
            for top in (F.MAXIMA if small else (10000,)):
                c = F.case(shape, pattern, top)
                levels, lut = M.tables(8 if top == 255 else 16, top)
                v = M.codes_to_input(c, s, levels, lut, "f32")[:, 0] * np.float32(levels)
                got = J.bicubic_codes(c, s, top)
                assert got.dtype == c.dtype and np.array_equal(got, np.rint(v).astype(c.dtype)), (shape, pattern, top)
                lost += int((v.astype(np.int64) != got).sum())
    assert lost > 0


# ---- the refusals of the C entries: on the host, before any HIP call -----------------------------------------------------------------

def jbu_refusals(lib, call):
    """call(**what differs) -> (status, message) of codon_jbu_upsample; shared with the GPU test"""
    for kw, word in J.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("jbu_upsample: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="jbu_upsample failed with status -1: jbu_upsample: "):
            L.check(st, "jbu_upsample")


def jbu_caller(lib, src, guide, tab, stab, out, ws, stream=None):
    """The good call of jbu_ref.REFUSALS -- u16 codes on a 5 x 7 plane at x4, guide rows of 28 bytes, images 560 apart -- over
    the given addresses, with what a refusal changes as keyword arguments"""
    P_ = C.c_void_p

    def call(B=1, h=5, w=7, src=src, fmt=L.FILL_U16, top=65535, guide=guide, row_bytes=28, image_bytes=560, scale=4, tab=tab,
             stab=stab, out=out, ws=ws, ws_bytes=None):
        need = B * lib.codon_jbu_workspace_bytes(h, w) if B > 0 else 0
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_jbu_upsample(B, h, w, p(src), fmt, top, p(guide), row_bytes, image_bytes, scale, p(tab), p(stab), p(out),
                                    p(ws), ws_bytes, stream)
        return st, lib.codon_last_error_string().decode()
    return call


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    assert lib.codon_jbu_workspace_bytes(5, 7) == 48 and lib.codon_jbu_workspace_bytes(65, 67) == (65 * 67 + 15) // 16 * 16
    assert lib.codon_jbu_workspace_bytes(0, 7) == 0 and lib.codon_jbu_workspace_bytes(5, 4097) == 0
    call = jbu_caller(lib, 4096, 8192, 12288, 16384, 20480, 24576)   # never dereferenced: every call is refused on the host
    jbu_refusals(lib, call)
    for kw in ({"src": 4097}, {"out": 20488}, {"tab": 12289}, {"stab": 16385}, {"ws": 24584}):
        assert "unaligned" in call(**kw)[1], kw
    p = C.c_void_p(4096)
    err = lib.codon_last_error_string
    up = lambda B=1, h=5, w=7, s=4, c=p, bits=8, lut=p, dm=255, wt=p, out=C.c_void_p(8192): lib.codon_lr_codes_upsample(  # noqa: E731
        B, h, w, s, c, bits, lut, dm, wt, out, None)
    assert up(c=None) == -1 and up(lut=None) == -1 and up(wt=None) == -1 and up(out=None) == -1 and b"null pointer" in err()
    assert err().startswith(b"lr_codes_upsample: ")
    assert up(s=5) == -2
    assert up(bits=12) == -1 and b"code_bits" in err()
    assert up(dm=256) == -1 and up(bits=16, dm=0) == -1 and up(bits=16, dm=65536) == -1 and b"depth_max" in err()
    assert up(B=0) == -1 and up(h=0) == -1 and up(w=-1) == -1
    assert up(out=C.c_void_p(4104)) == -1 and b"aligned" in err()
    assert up(bits=16, dm=4096, c=C.c_void_p(4097)) == -1 and b"aligned" in err()
    assert up(out=p) == -1 and b"same buffer" in err()


# ---- the command line ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("argv, word", [
    (["--baseline", "jbu", "--input-depth", "a"], "--baseline needs --lr-depth (it is refused with --input-depth"),
    (["--baseline", "bicubic", "--lr-depth", "a", "--weights", "w.pth"], "--baseline is refused with --weights"),
    (["--baseline", "bicubic", "--lr-depth", "a", "--weights", "w.pth", "--ema"], "--baseline is refused with --weights"),
    (["--baseline", "jbu", "--lr-depth", "a", "--ema"], "--baseline is refused with --ema"),
    (["--baseline", "jbu", "--lr-depth", "a", "--self-ensemble"], "--baseline is refused with --self-ensemble"),
    (["--lr-depth", "a", "--jbu-sigma-s", "1.5"], "--jbu-sigma-s needs --baseline jbu"),
    (["--lr-depth", "a", "--baseline", "bicubic", "--jbu-sigma-r", "5"], "--jbu-sigma-r needs --baseline jbu"),
    (["--lr-depth", "a", "--baseline", "jbu", "--jbu-sigma-s", "0"], "--jbu-sigma-s 0.0 must be positive"),
    (["--lr-depth", "a", "--baseline", "jbu", "--jbu-sigma-r", "-2"], "--jbu-sigma-r -2.0 must be positive"),
    (["--lr-depth", "a", "--baseline", "nearest"], "invalid choice"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        infer.main(["--input-color", "c", *argv])
    assert e.value.code == 2 and word in capsys.readouterr().err


def test_run_loop_refusals_without_gpu():
    kw = dict(lr_depth="b", scale=4)
    with pytest.raises(ValueError, match="run_loop: baseline 'nearest'"):
        infer.run_loop(None, None, torch.float32, None, "c", baseline="nearest", **kw)
    with pytest.raises(ValueError, match="run_loop: baseline needs lr_depth"):
        infer.run_loop(None, None, torch.float32, "a", "c", baseline="jbu")
    with pytest.raises(ValueError, match="run_loop: baseline with self_ensemble"):
        infer.run_loop(None, None, torch.float32, None, "c", baseline="jbu", self_ensemble=True, **kw)
    with pytest.raises(ValueError, match="run_loop: sigma_s 0"):
        infer.run_loop(None, None, torch.float32, None, "c", baseline="jbu", jbu_sigma_s=0, **kw)
    with pytest.raises(ValueError, match="run_loop: fill_sigma -1"):
        infer.run_loop(None, None, torch.float32, None, "c", baseline="jbu", jbu_sigma_r=-1, **kw)
    with pytest.raises(ValueError, match="run_loop: model is None without a baseline"):
        infer.run_loop(None, None, torch.float32, None, "c", **kw)
