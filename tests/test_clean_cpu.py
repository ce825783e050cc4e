"""The outlier rejection's definition (tests/clean_ref.py) on the CPU: what the definition promises -- an output
code is the input's or 0, the identity with both rules off, symmetry under flips and the transpose, the link's bound to the code,
the two sides of rule 2's threshold, diagonal neighbours that support but do not connect -- the committed scene's counts, one
end-to-end property through the registration's restatement, and every refusal that needs no GPU: of Cleaner, of the C entry
(validated on the host before any HIP call) and of both command lines.  Expectations are spelled out here, not derived from the
code under test."""
import ctypes as C
import re

import numpy as np
import pytest

from codon_amd import _lib as L
from codon_amd import clean as K
from codon_amd import register as P
from tests import clean_ref as R
from tests import register_ref as G

RQ = 1311                                   # rint(65536 * 0.02)
FORMATS = ((np.uint8, 255), (np.uint16, 65535), (np.uint16, 10000))


def _random(h, w, top, dtype, seed):
    """30 % holes, a few levels with jitter: components of many sizes"""
    g = np.random.default_rng(seed)
    c = g.choice([top // 5, top // 5 + 1, top // 2, top // 2 + 2, top - 1], size=(h, w))
    c[g.random((h, w)) < 0.3] = 0
    return c.astype(dtype)


def _union_find(k, A, Rq):
    """An independent labelling of one small plane: a sequential union-find over the right and down links, in Python integers"""
    h, w = k.shape
    parent = list(range(h * w))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    def link(a, b):
        a, b = int(a), int(b)
        return a != 0 and b != 0 and abs(a - b) <= A + ((Rq * min(a, b)) >> 16)

    for i in range(h):
        for j in range(w):
            for ii, jj in ((i, j + 1), (i + 1, j)):
                if ii < h and jj < w and link(k[i, j], k[ii, jj]):
                    a, b = find(i * w + j), find(ii * w + jj)
                    parent[max(a, b)] = min(a, b)
    return np.array([find(p) if k.flat[p] != 0 else -1 for p in range(h * w)]).reshape(h, w)


def test_rel_q16_and_the_defaults():
    assert R.rel_q16(0.02) == RQ == K.rel_q16("t", 0.02) and R.rel_q16(0.0) == 0 and K.rel_q16("t", 0.99999) == 65535
    assert R.DEFAULTS == K.DEFAULTS == dict(tolerance=2, tolerance_rel=0.02, min_support=3, min_region=16)
    c = K.Cleaner()
    assert (c.tolerance, c.tolerance_rel_q16, c.min_support, c.min_region) == (2, RQ, 3, 16)
    assert R.STATS == K.STATS == ("valid", "flying", "speckle", "regions")
    assert (R.MAX_SUPPORT, R.MAX_REGION, R.MAX_REL) == (K.MAX_SUPPORT, K.MAX_REGION, K.MAX_REL_Q16) == (8, 1 << 24, 65535)


@pytest.mark.parametrize("dtype, top", FORMATS, ids=["u8", "u16", "u16_10000"])
def test_an_output_code_is_the_input_or_zero(dtype, top):
    c = _random(23, 31, top, dtype, 3)
    for A, Rq, Kk, N in ((2, RQ, 3, 16), (0, RQ, 1, 4), (5, 0, 8, 2), (1, RQ, 0, 23 * 31)):
        out, stats = R.clean_plane(c, A, Rq, Kk, N)
        assert out.dtype == c.dtype and ((out == c) | (out == 0)).all() and (out[c == 0] == 0).all()
        valid, flying, speckle, regions = (int(v) for v in stats)
        assert valid == (c != 0).sum() and flying + speckle == ((c != 0) & (out == 0)).sum()
        assert regions <= speckle <= regions * max(N - 1, 0)


@pytest.mark.parametrize("dtype, top", FORMATS, ids=["u8", "u16", "u16_10000"])
def test_both_rules_off_is_the_identity(dtype, top):
    c = _random(17, 19, top, dtype, 4)
    for N in (0, 1):
        out, stats = R.clean_plane(c, 2, RQ, 0, N)
        assert out.tobytes() == c.tobytes() and stats.tolist() == [int((c != 0).sum()), 0, 0, 0]


def test_the_labelling_is_an_independent_union_finds():
    """components -- vectorised, labels travelling along the right and down links -- gives the partition, and the smallest index
    as the label, of a sequential union-find written out here"""
    for seed, (h, w) in enumerate(((1, 1), (1, 9), (7, 1), (12, 13), (16, 21))):
        k = _random(h, w, 10000, np.uint16, 20 + seed).astype(np.int64)
        assert np.array_equal(R.components(k, 2, RQ), _union_find(k, 2, RQ)), (h, w)
    snake = R.plane((1, 17, 17), "serpentine", 10000)[0].astype(np.int64)
    lab = R.components(snake, 2, RQ)
    assert np.array_equal(lab, _union_find(snake, 2, RQ)) and set(np.unique(lab)) == {-1, 0}


@pytest.mark.parametrize("square", [False, True], ids=["oblong", "square"])
def test_the_result_commutes_with_flips_and_the_transpose(square):
    """The restatement unites right and down only: an asymmetry of its own would show here"""
    h, w = (21, 21) if square else (18, 27)
    g = np.random.default_rng(5)            # a quarter holes, one level in three pixels of five: components from 1 pixel to dozens
    c = g.choice([0, 2000, 2001, 5000], size=(h, w), p=[0.25, 0.3, 0.3, 0.15]).astype(np.uint16)
    for params in ((2, RQ, 3, 16), (2, RQ, 0, 5), (0, RQ, 2, 40)):
        out, stats = R.clean_plane(c, *params)
        assert 0 < (out != 0).sum() < (c != 0).sum()
        views = [lambda a: a[::-1], lambda a: a[:, ::-1], lambda a: a[::-1, ::-1]] + ([lambda a: a.T] if square else [])
        for view in views:
            o2, s2 = R.clean_plane(np.ascontiguousarray(view(c)), *params)
            assert np.array_equal(o2, view(out)) and np.array_equal(s2, stats)


@pytest.mark.parametrize("v", [10, 40000])
def test_the_link_holds_at_tau_and_not_one_beyond(v):
    """A = 2, Rq = 1311: tau(10) = 2 + (13110 >> 16) = 2, tau(40000) = 2 + (52440000 >> 16) = 2 + 800"""
    tau = {10: 2, 40000: 802}[v]
    assert 2 + ((RQ * v) >> 16) == tau
    for d, want in ((tau, True), (tau + 1, False)):
        a, b = np.array([v], dtype=np.int64), np.array([v + d], dtype=np.int64)
        assert bool(R.linked(a, b, 2, RQ)[0]) is want and bool(R.linked(b, a, 2, RQ)[0]) is want
        pair = np.array([[v, v + d]], dtype=np.uint16)
        out, stats = R.clean_plane(pair, 2, RQ, 1, 0)             # rule 1 with K = 1: a linked pair supports itself
        assert (out != 0).all() == want and stats.tolist() == [2, 0 if want else 2, 0, 0]
        out, stats = R.clean_plane(pair, 2, RQ, 0, 2)             # rule 2 with N = 2: a linked pair is one component of 2
        assert (out != 0).all() == want and stats.tolist() == [2, 0, 0 if want else 2, 0 if want else 2]
    assert not R.linked(np.array([0]), np.array([1]), 65535, 65535)[0]            # a hole is linked to nothing


def test_blobs_on_either_side_of_rule_2():
    N = 16
    c = np.zeros((12, 20), dtype=np.uint16)
    c[2:6, 2:6] = 500                       # 16 pixels
    c[2:6, 10:14] = 500
    c[2, 10] = 0                            # 15 pixels
    out, stats = R.clean_plane(c, 2, RQ, 0, N)
    assert (out[2:6, 2:6] == 500).all() and not out[:, 8:].any() and stats.tolist() == [31, 0, 15, 1]
    out, stats = R.clean_plane(c, 2, RQ, 0, N + 1)
    assert not out.any() and stats.tolist() == [31, 0, 31, 2]
    out, stats = R.clean_plane(c, 2, RQ, 3, N)                      # and rule 1 takes nothing from either: every pixel has 3
    assert stats.tolist() == [31, 0, 15, 1]


def test_diagonal_blobs_are_two_components_that_support_each_other():
    c = np.zeros((6, 6), dtype=np.uint16)
    c[1:3, 1:3] = 700                       # two 2 x 2 blobs that touch at one corner only
    c[3:5, 3:5] = 700
    lab = R.components(c.astype(np.int64), 2, RQ)
    assert set(np.unique(lab)) == {-1, 7, 21}
    assert R.clean_plane(c, 2, RQ, 0, 5)[1].tolist() == [8, 0, 8, 2]                 # 4 + 4, never one component of 8
    assert R.clean_plane(c, 2, RQ, 0, 4)[1].tolist() == [8, 0, 0, 0]
    n = R.support(c.astype(np.int64), 2, RQ)
    assert n[2, 2] == 4 and n[3, 3] == 4 and n[1, 1] == 3                            # the corner pixels count each other
    out, stats = R.clean_plane(c, 2, RQ, 4, 0)
    assert (out != 0).sum() == 2 and out[2, 2] == 700 and out[3, 3] == 700 and stats.tolist() == [8, 6, 0, 0]


def test_one_pixel_and_the_constant_plane():
    one = np.array([[9]], dtype=np.uint8)
    for Kk in (1, 3, 8):
        assert R.clean_plane(one, 2, RQ, Kk, 0)[0][0, 0] == 0
    for N in (0, 1):
        assert R.clean_plane(one, 2, RQ, 0, N)[0][0, 0] == 9
    assert R.clean_plane(one, 2, RQ, 0, 2)[1].tolist() == [1, 0, 1, 1]
    for h, w in ((2, 2), (2, 5), (9, 4)):
        c = np.full((h, w), 1234, dtype=np.uint16)
        out, stats = R.clean_plane(c, 0, 0, 3, min(16, h * w))
        assert (out == 1234).all() and stats.tolist() == [h * w, 0, 0, 0]
    c = np.full((6, 7), 1234, dtype=np.uint16)                       # K > 3 takes the corners, K > 5 the border
    assert (R.clean_plane(c, 0, 0, 4, 0)[0] == 0).sum() == 4
    out = R.clean_plane(c, 0, 0, 6, 0)[0]
    assert (out[1:-1, 1:-1] == 1234).all() and (out != 0).sum() == 4 * 5


@pytest.mark.parametrize("top", [10000, 65535, 255])
def test_the_scene_counts(top):
    """The prototype's result on the committed scene, on all three grids: of 3853 valid pixels all 132 planted flying pixels and
    the 1-pixel blob go under rule 1, 28 speckle pixels go in 3 regions, the 16-pixel blob stays, no pixel of either surface is
    lost; with rule 1 off rule 2 removes the ring itself, as 130 tiny regions (123 on the 8-bit grid)"""
    c = R.scene(top)
    A = {10000: 8, 65535: 52, 255: 1}[top]
    ring, blobs = R.ring_mask(), R.blob_mask()
    assert ring.sum() == 132 and blobs.sum() == 45 and (c != 0).sum() == 3853
    assert ((c == 0) == (np.pad(np.ones((24, 8), bool), ((8, 8), (61, 31))) & ~blobs)).all()
    out, stats = R.clean_plane(c, A, RQ, 3, 16)
    assert stats.tolist() == [3853, 133, 28, 3]
    assert not out[ring].any()
    big = np.zeros_like(blobs)
    big[9:13, 62:66] = True                                         # the 16-pixel blob
    assert (out[big] == c[big]).all() and not out[blobs & ~big].any()
    surfaces = (c != 0) & ~ring & ~blobs
    assert (out[surfaces] == c[surfaces]).all()
    out0, stats0 = R.clean_plane(c, A, RQ, 0, 16)
    in_ring = 130 if top != 255 else 123
    assert stats0.tolist() == [3853, 0, 132 + 1 + 4 + 9 + 15, in_ring + 4]
    assert not out0[ring].any() and (out0[surfaces] == c[surfaces]).all() and (out0[big] == c[big]).all()
    lab = R.components(c.astype(np.int64), A, RQ)
    assert len(np.unique(lab[ring])) == in_ring == R.SCENE_RING_REGIONS[top]


def test_cleaning_keeps_flying_pixels_out_of_the_registered_map():
    """The scene through the registration's restatement with a rig that translates sideways only (z is unchanged): without
    cleaning the registered map holds codes strictly between the two surfaces' bands, with cleaning none"""
    c = R.scene(10000)
    h, w = c.shape
    A = G.ray_table(h, w, 100.0, 100.0, (w - 1) / 2, (h - 1) / 2, (0.0,) * 5, np.eye(3))
    T = G.translation_q20((0.05, 0.0, 0.0), 0.001)                  # 50 codes to the side
    proj = G.projection_q8(100.0, 100.0, (w - 1) / 2, (h - 1) / 2, 1)
    between = lambda m: int(((m > R.NEAR_BAND[1]) & (m < R.FAR_BAND[0])).sum())      # noqa: E731
    raw, _ = G.register_plane(c, A, T, proj, h, w, 10000)
    cleaned, stats = R.clean_plane(c, 8, RQ, 3, 16)
    reg, _ = G.register_plane(cleaned, A, T, proj, h, w, 10000)
    assert set(np.unique(raw)) <= set(np.unique(c)) | {0}           # z is unchanged
    print(f"codes between the surfaces in the registered map: {between(raw)} without cleaning, {between(reg)} with")
    assert between(c) == 132 and between(raw) > 0 and between(reg) == 0
    assert (reg != 0).sum() > 0.9 * (raw != 0).sum()


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, word", [
    (dict(tolerance=-1), "tolerance -1 "), (dict(tolerance=65536), "tolerance 65536 "), (dict(tolerance=2.0), "tolerance 2.0 "),
    (dict(tolerance=True), "tolerance True "), (dict(tolerance_rel=-0.01), "tolerance_rel -0.01 "),
    (dict(tolerance_rel=1.0), "tolerance_rel 1.0 "), (dict(tolerance_rel=0.999999), "tolerance_rel 0.999999 "),
    (dict(tolerance_rel=float("nan")), "tolerance_rel nan "), (dict(tolerance_rel="x"), "tolerance_rel 'x' "),
    (dict(min_support=-1), "min_support -1 "), (dict(min_support=9), "min_support 9 "), (dict(min_support=3.0), "min_support 3.0 "),
    (dict(min_region=-1), "min_region -1 "), (dict(min_region=(1 << 24) + 1), "min_region 16777217 "),
    (dict(min_region=None), "min_region None "),
])
def test_cleaner_refusals(kw, word):
    with pytest.raises(ValueError, match="Cleaner: " + re.escape(word)):
        K.Cleaner(**kw)


def test_cleaner_accepts_the_bounds():
    c = K.Cleaner(0, 0.0, 0, 0)
    assert (c.tolerance, c.tolerance_rel_q16, c.min_support, c.min_region) == (0, 0, 0, 0)
    c = K.Cleaner(65535, 65535 / 65536, 8, 1 << 24)
    assert (c.tolerance, c.tolerance_rel_q16, c.min_support, c.min_region) == (65535, 65535, 8, 1 << 24)


def clean_refusals(lib, call):
    """call(**what differs) -> (status, message) of codon_clean_depth; shared with the GPU test"""
    for kw, word in R.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("clean_depth: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="clean_depth failed with status -1: clean_depth: "):
            L.check(st, "clean_depth")


def clean_caller(lib, src, out, ws, counts=None, stream=None):
    """The good call of clean_ref.REFUSALS -- u16 codes, a 5 x 7 plane, the defaults -- over the given addresses, with what a
    refusal changes as keyword arguments"""
    P_ = C.c_void_p

    def call(B=1, h=5, w=7, src=src, fmt=L.FILL_U16, top=65535, tol_abs=2, tol_rel=RQ, support=3, region=16, out=out, counts=counts,
             ws=ws, ws_bytes=None):
        need = lib.codon_clean_workspace_bytes(B, h, w)
        ws_bytes = need if ws_bytes is None else need - 1
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_clean_depth(B, h, w, p(src), fmt, top, tol_abs, tol_rel, support, region, p(out), p(counts), p(ws), ws_bytes,
                                   stream)
        return st, lib.codon_last_error_string().decode()
    return call


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    q = lib.codon_clean_workspace_bytes
    assert q(1, 5, 7) == 2 * 36 * 4 and q(3, 5, 7) == 3 * 2 * 36 * 4 and q(8, 424, 512) == 8 * 424 * 512 * 8
    assert q(0, 5, 7) == 0 and q(65536, 5, 7) == 0 and q(1, 0, 7) == 0 and q(1, 5, 4097) == 0 and q(1, 4096, 4096) == 8 << 24
    call = clean_caller(lib, 4096, 12288, 16384)                    # never dereferenced: every call is refused on the host
    clean_refusals(lib, call)
    for kw in ({"src": 4097}, {"out": 12289}, {"counts": 20482}, {"ws": 16392}):
        assert "unaligned" in call(**kw)[1], kw
    # at the bounds themselves the refusal is the short workspace asked for beside them: no bound is off by one
    at = dict(top=10000, tol_abs=10000, tol_rel=65535, support=8, region=1 << 24, ws_bytes="short")
    assert "too small" in call(**at)[1]
    assert "too small" in call(tol_abs=0, tol_rel=0, support=0, region=0, ws_bytes="short")[1]


NEEDED = ["--depth", "d", "--out", "o"]


@pytest.mark.parametrize("argv, word", [
    (["--out", "o"], "the following arguments are required: --depth"),
    (["--depth", "d"], "the following arguments are required: --out"),
    ([*NEEDED, "--depth-bits", "12"], "invalid choice"),
    ([*NEEDED, "--depth-max", "10000"], "--depth-max needs --depth-bits 16"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "0"], "--depth-max 0 must be in \\[1, 65535\\]"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "65536"], "--depth-max 65536 must be in"),
    (["--depth", "d", "--out", "./d"], "--out is --depth"),
    ([*NEEDED, "--tolerance", "-1"], "--tolerance -1 "),
    ([*NEEDED, "--tolerance", "256"], "--tolerance 256 is above the largest code 255"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "10000", "--tolerance", "10001"], "--tolerance 10001 is above the largest code 10000"),
    ([*NEEDED, "--tolerance", "1.5"], "invalid int value"),
    ([*NEEDED, "--tolerance-rel", "1.0"], "--tolerance-rel 1.0 "),
    ([*NEEDED, "--tolerance-rel", "-0.5"], "--tolerance-rel -0.5 "),
    ([*NEEDED, "--tolerance-rel", "nan"], "--tolerance-rel nan "),
    ([*NEEDED, "--min-support", "9"], "--min-support 9 "),
    ([*NEEDED, "--min-support", "-1"], "--min-support -1 "),
    ([*NEEDED, "--min-region", "-1"], "--min-region -1 "),
    ([*NEEDED, "--min-region", "16777217"], "--min-region 16777217 "),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        K.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_command_line_defaults(tmp_path, capsys):
    a, _, cleaner = K.parse_args(NEEDED)
    assert (a.depth_bits, a.depth_max, a.tolerance, a.tolerance_rel, a.min_support, a.min_region, a.stats) == (8, None, 2, 0.02, 3, 16, False)
    assert (cleaner.tolerance, cleaner.tolerance_rel_q16, cleaner.min_support, cleaner.min_region) == (2, RQ, 3, 16)
    a, _, cleaner = K.parse_args([*NEEDED, "--depth-bits", "16", "--depth-max", "10000", "--tolerance", "8", "--tolerance-rel", "0.05",
                                  "--min-support", "0", "--min-region", "40", "--stats"])
    assert (a.depth_bits, a.depth_max, a.stats) == (16, 10000, True)
    assert (cleaner.tolerance, cleaner.tolerance_rel_q16, cleaner.min_support, cleaner.min_region) == (8, 3277, 0, 40)
    with pytest.raises(SystemExit) as e:                                 # the directory is looked at before the GPU is asked for
        K.main(["--depth", str(tmp_path / "none"), "--out", str(tmp_path / "o")])
    assert e.value.code == 2 and "is not a directory" in capsys.readouterr().err


REG = ["--depth", "d", "--calib", "c.json", "--out", "o"]


@pytest.mark.parametrize("argv, word", [
    ([*REG, "--clean-tolerance", "3"], "--clean-tolerance needs --clean"),
    ([*REG, "--clean-tolerance-rel", "0.1"], "--clean-tolerance-rel needs --clean"),
    ([*REG, "--clean-min-support", "2"], "--clean-min-support needs --clean"),
    ([*REG, "--clean-min-region", "0"], "--clean-min-region needs --clean"),
    ([*REG, "--clean", "--clean-tolerance", "-1"], "--clean-tolerance -1 "),
    ([*REG, "--clean", "--clean-tolerance", "256"], "--clean-tolerance 256 is above the largest code 255"),
    ([*REG, "--clean", "--clean-tolerance-rel", "1.0"], "--clean-tolerance-rel 1.0 "),
    ([*REG, "--clean", "--clean-min-support", "9"], "--clean-min-support 9 "),
    ([*REG, "--clean", "--clean-min-region", "16777217"], "--clean-min-region 16777217 "),
])
def test_register_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        P.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_register_command_line_clean_is_off_by_default():
    a, _ = P.parse_args(REG)
    assert a.clean is False and a.cleaner is None
    a, _ = P.parse_args([*REG, "--clean"])
    c = a.cleaner
    assert a.clean and (c.tolerance, c.tolerance_rel_q16, c.min_support, c.min_region) == (2, RQ, 3, 16)
    a, _ = P.parse_args([*REG, "--clean", "--clean-tolerance", "8", "--clean-tolerance-rel", "0", "--clean-min-support", "0",
                         "--clean-min-region", "1", "--depth-bits", "16"])
    c = a.cleaner
    assert (c.tolerance, c.tolerance_rel_q16, c.min_support, c.min_region) == (8, 0, 0, 1)
