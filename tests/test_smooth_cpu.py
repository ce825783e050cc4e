"""The spatial smoothing of sensor depth maps without a GPU: the numpy restatement tests/smooth_ref.py, which the kernel
of csrc/smooth.hip is held to bit for bit (tests/test_gpu_smooth.py, tools/host_check.py smooth), is pinned here by the properties
the definition promises; then the seeded scene, the launch rule against the library's own, and every refusal by name."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import register as P
from codon_amd import smooth as K
from tests import clean_ref
from tests import smooth_ref as R

RQ = R.RQ


def _random(h, w, top, holes, seed):
    """A slanted surface with noise of about tau and a far block, `holes` of it missing"""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    c = top // 3 + (top // 200 + 1) * (x + 2 * y) // 3 + g.integers(-3, 4, size=(h, w))
    c[h // 3:h // 2, w // 4:w // 2] += top // 3
    c = np.clip(c, 1, top)
    c[g.random((h, w)) < holes] = 0
    return c.astype(np.uint8 if top == 255 else np.uint16)


def test_the_defaults_and_the_names():
    assert R.DEFAULTS == K.DEFAULTS == dict(radius=2, passes=2, sigma=None, tolerance=2, tolerance_rel=0.02, pairs=True)
    assert R.STATS == K.STATS == ("valid", "changed", "alone", "max")
    assert (R.MAX_RADIUS, R.MAX_PASSES) == (K.MAX_RADIUS, K.MAX_PASSES) == (4, 3)
    f = K.Smoother()
    assert (f.radius, f.passes, f.sigma, f.tolerance, f.tolerance_rel_q16, f.pairs) == (2, 2, None, 2, RQ, True)
    assert R.linked is clean_ref.linked and RQ == 1311
    assert K.stats_line(np.array([5, 4, 3, -1], dtype=np.int32)) == "valid=5 changed=4 alone=3 max=4294967295"


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("sigma", [None, 0.8, 1.5, 40.0])
def test_the_weight_table(radius, sigma):
    """Values, the centre, the point symmetry; the module's table is the restatement's; 2N + D stays below 2^32"""
    W = K.weight_table(radius, sigma)
    side = 2 * radius + 1
    assert W.shape == (side, side) and W.dtype == np.int32 and np.array_equal(W, R.weight_table(radius, sigma))
    assert W[radius, radius] == 256 and W.min() >= 0 and W.max() == 256
    assert np.array_equal(W, W[::-1, ::-1]) and np.array_equal(W, W.T)
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            want = 256 if sigma is None else int(np.rint(256.0 * np.exp(-(dy * dy + dx * dx) / (2.0 * sigma * sigma))))
            assert W[dy + radius, dx + radius] == want
    if sigma == 0.8 and radius >= 2:
        assert W[0, 0] == 0 and W[radius, radius - 1] > 0                # zero-weight corners
    assert 2 * 65535 * int(W.sum()) + int(W.sum()) < 1 << 32


@pytest.mark.parametrize("top", [255, 10000, 65535])
def test_holes_stay_codes_move_by_at_most_tau_and_passes_compose(top):
    c = _random(37, 41, top, 0.2, 3)
    before = c.copy()
    for R_, sigma, A, Rq, pairs in ((1, None, 2, RQ, True), (2, 0.8, 0, 0, False), (4, 1.5, 5, 3000, True), (3, None, top, 0, False)):
        cur = c
        for passes in (1, 2, 3):
            out, stats = R.smooth(c[None], R_, passes, sigma, A, Rq, pairs)
            step, _ = R.smooth(cur[None], R_, 1, sigma, A, Rq, pairs)
            assert np.array_equal(out[0], step[0]), "passes=P is passes=1 applied P times"
            assert out.dtype == c.dtype and np.array_equal(out[0] == 0, c == 0), "the hole set"
            move = np.abs(step[0].astype(np.int64) - cur.astype(np.int64))
            assert (move <= R.tau(cur, A, Rq)).all(), "one pass moves a code by at most tau(c_p)"
            d = np.abs(out[0].astype(np.int64) - c.astype(np.int64))
            assert stats.tolist() == [[(c != 0).sum(), (d != 0).sum(), stats[0, 2], d.max()]]
            cur = step[0]
        assert stats[0, 1] > 0 or A == 0
    assert np.array_equal(c, before)


def test_alone_counts_the_first_pass():
    """Three codes in a row, the outer two linked to the middle one and not to each other: with the pair rule the middle has a
    pair and the ends nothing; a lone code far from everything is alone either way"""
    c = np.array([[100, 102, 104, 0, 0, 0, 0, 0, 9000]], dtype=np.uint16)
    out, stats = R.smooth(c[None], 1, 1, None, 2, 0, True)
    assert out[0].tolist() == [[100, 102, 104, 0, 0, 0, 0, 0, 9000]] and stats.tolist() == [[4, 0, 3, 0]]
    out, stats = R.smooth(c[None], 1, 1, None, 2, 0, False)
    assert out[0].tolist() == [[101, 102, 103, 0, 0, 0, 0, 0, 9000]] and stats.tolist() == [[4, 2, 1, 1]]
    out, stats = R.smooth(c[None], 1, 3, None, 2, 0, False)           # half rounds up: 101 102 103 -> 102 102 103, which stays; the count is the first pass's
    assert stats[0, 2] == 1 and out[0, 0, :3].tolist() == [102, 102, 103]


def test_rounding_is_half_up_and_weights_are_applied():
    c = np.array([[10, 11]], dtype=np.uint8)
    assert R.smooth(c[None], 1, 1, None, 2, 0, False)[0][0].tolist() == [[11, 11]]          # 10.5 -> 11
    c = np.array([[10, 13, 10]], dtype=np.uint8)
    W = R.weight_table(1, 0.8)[1, 0]                                  # 117
    want = (2 * (256 * 13 + 2 * W * 10) + 256 + 2 * W) // (2 * (256 + 2 * W))
    assert R.smooth(c[None], 1, 1, 0.8, 3, 0, True)[0][0, 0, 1] == want == 12


@pytest.mark.parametrize("gy, gx", [(3, 7), (-5, 2), (0, 11)])
def test_a_cut_plane_comes_back_bit_for_bit_with_the_pair_rule_and_not_without(gy, gx):
    """A noiseless plane with an integer gradient, cut by 10 % random holes and by an occluder further away than tau: R = 3,
    sigma = 1.5, P = 1 .. 3.  With the rule off the same plane does NOT come back, which keeps the first assertion from being vacuous"""
    h, w, A = 48, 56, 16
    y, x = np.mgrid[0:h, 0:w]
    c = 20000 + gy * y + gx * x
    c[10:30, 15:40] = 40000 + 9 * x[10:30, 15:40]                     # the occluder: another plane, 20000 codes away
    g = np.random.default_rng(11)
    c[g.random((h, w)) < 0.1] = 0
    c = c.astype(np.uint16)
    assert A >= max(abs(gy), abs(gx), 9) and 3 * (abs(gy) + abs(gx)) > A     # neighbours are linked; the window's far corners are not
    for passes in (1, 2, 3):
        out, stats = R.smooth(c[None], 3, passes, 1.5, A, 0, True)
        assert np.array_equal(out[0], c) and stats[0, 1] == 0 and stats[0, 3] == 0
        off, stats = R.smooth(c[None], 3, passes, 1.5, A, 0, False)
        assert not np.array_equal(off[0], c) and stats[0, 1] > 50


def test_a_step_larger_than_tau_is_unchanged_on_both_sides():
    for top, lo, hi in ((255, 100, 110), (10000, 4000, 4200), (65535, 30000, 40000)):
        c = np.full((20, 24), lo, dtype=np.uint8 if top == 255 else np.uint16)
        c[:, 11:] = hi
        assert hi - lo > R.tau(lo, 2, RQ)
        for pairs in (True, False):
            out, stats = R.smooth(c[None], 4, 3, None, 2, RQ, pairs)
            assert np.array_equal(out[0], c) and stats[0, [0, 1, 3]].tolist() == [480, 0, 0]


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------------

# measured with this file (DESIGN 12.25 records them): MAE in codes over the valid pixels, against the noiseless codes
SCENE_MAE = {255: (1.52, 0.31), 10000: (6.02, 0.98)}                   # top: (the input's, the defaults')
SCENE_MAE_NO_PAIRS = 3.70                                               # top 10000, the defaults with the pair rule off


@pytest.mark.parametrize("top", [255, 10000])
def test_the_scene(top):
    """96 x 128, a slanted background and a steeper slanted rectangle, uniform noise, 5 % holes: at the defaults the error against
    the noiseless codes must fall below the input's -- a condition; the measured figures are printed and pinned to two digits"""
    noisy, clean = R.scene(top)
    assert noisy.shape == (96, 128) and 0.03 < (noisy == 0).mean() < 0.07
    out, stats = R.smooth(noisy[None])
    before, after = R.mae(noisy, clean), R.mae(out[0], clean)
    print(f"top {top}: MAE {before:.3f} -> {after:.3f}, stats {stats[0].tolist()}")
    assert after < before
    assert np.array_equal(out[0] == 0, noisy == 0)
    assert (round(before, 2), round(after, 2)) == SCENE_MAE[top]
    if top == 10000:
        plain, _ = R.smooth(noisy[None], pairs=False)
        worse = R.mae(plain[0], clean)
        print(f"top {top}: MAE without the pair rule {worse:.3f}")
        assert after < worse and round(worse, 2) == SCENE_MAE_NO_PAIRS


# ---- the launch rule and the case set ---------------------------------------------------------------------------------------------------

def test_the_launch_rule_is_the_librarys():
    """tests/smooth_ref.fuse_bound restates csrc/launch_rules.h; the library's own answer, asked without a launch"""
    for radius in (1, 2, 3, 4):
        for passes in (1, 2, 3):
            p = K.plan(radius, passes)
            assert p == dict(tile=R.TILE, fuse_bound=R.fuse_bound(radius), fused=min(passes, R.fuse_bound(radius)),
                             launches=R.launches(radius, passes)), (radius, passes)
    q = L.load().codon_smooth_plan
    assert [q(r, p, None) for r, p in ((0, 1), (5, 1), (1, 0), (1, 4))] == [0] * 4
    with pytest.raises(ValueError, match="smooth_plan: radius 5"):
        K.plan(5, 1)


def test_what_the_case_set_covers():
    rows = R.cases()
    assert len(rows) == len(R.PLANES) * 18 == 144 and len(set(rows)) == 144
    col = lambda i: {r[i] for r in rows}                                  # noqa: E731
    assert col(0) == {1, 3} and {r[1:3] for r in rows} == set(R.PLANES)
    assert col(3) == {1, 2, 4} and col(4) == {1, 2, 3} and col(5) == {None, 0.8} and col(6) == {True, False}
    assert col(9) == set(R.PATTERNS) and col(10) == {255, 10000, 65535}
    for plane in R.PLANES:
        mine = [r for r in rows if r[1:3] == plane]
        assert {(r[3], r[4], r[6]) for r in mine} == {(a, b, c) for a in R.RADII for b in R.PASSES for c in (True, False)}
    for top in R.FORMATS:
        assert {(r[7], r[8]) for r in rows if r[10] == top} == {(0, 0), (2, RQ), (top, 0)}
        assert {r[9] for r in rows if r[10] == top} == set(R.PATTERNS)
    # both sides of the fusion bound: calls that are one launch of several passes, and calls of several launches
    assert any(r[4] > 1 and R.launches(r[3], r[4]) == 1 for r in rows) and any(R.launches(r[3], r[4]) > 1 for r in rows)
    assert any(R.codes_of(r).max() >= 32768 for r in rows)
    changed = sum(int(R.want(r)[1][:, 1].sum()) > 0 for r in rows)
    alone = sum(int(R.want(r)[1][:, 2].sum()) > 0 for r in rows)
    assert changed > 40 and alone > 30, (changed, alone)
    assert any(r[5] == 0.8 and r[3] >= 2 for r in rows)                  # a table with zero-weight corners


# ---- refusals by name -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, word", [
    ({"radius": 0}, "radius 0 (an integer in 1..4)"), ({"radius": 5}, "radius 5 (an integer in 1..4)"),
    ({"radius": True}, "radius True"), ({"radius": 2.0}, "radius 2.0"),
    ({"passes": 0}, "passes 0 (an integer in 1..3)"), ({"passes": 4}, "passes 4 (an integer in 1..3)"), ({"passes": False}, "passes False"),
    ({"sigma": 0}, "sigma 0 (None, or a finite positive number of pixels)"), ({"sigma": -1.5}, "sigma -1.5"),
    ({"sigma": float("inf")}, "sigma inf"), ({"sigma": float("nan")}, "sigma nan"), ({"sigma": True}, "sigma True"),
    ({"sigma": "wide"}, "sigma 'wide'"),
    ({"tolerance": -1}, "tolerance -1"), ({"tolerance": 65536}, "tolerance 65536"), ({"tolerance": True}, "tolerance True"),
    ({"tolerance_rel": 1.0}, "tolerance_rel 1.0"), ({"tolerance_rel": -0.1}, "tolerance_rel -0.1"), ({"tolerance_rel": True}, "tolerance_rel True"),
    ({"pairs": 1}, "pairs 1 (True or False)"),
])
def test_smoother_refusals(kw, word):
    with pytest.raises(ValueError, match="Smoother: " + re.escape(word)):
        K.Smoother(**kw)


def test_call_refusals_come_before_the_device():
    f = K.Smoother(tolerance=300)
    with pytest.raises(ValueError, match="smooth_depth: tolerance 300 above the largest code 255"):
        f(torch.zeros((4, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="smooth_depth: tolerance 300 above the largest code 100"):
        f(torch.zeros((4, 5), dtype=torch.int16), 100)
    with pytest.raises(ValueError, match="smooth_depth: depth_max 10000 with 8-bit codes"):
        K.Smoother()(torch.zeros((4, 5), dtype=torch.uint8), 10000)
    with pytest.raises(RuntimeError, match="smooth_depth expects"):
        K.Smoother()(torch.zeros((4, 5), dtype=torch.float32))
    with pytest.raises(ValueError, match="smooth_depth: an empty map"):
        K.Smoother()(torch.zeros((0, 5), dtype=torch.uint8))
    with pytest.raises(ValueError, match="weight_table: radius 5"):
        K.weight_table(5)
    with pytest.raises(ValueError, match="weight_table: sigma 0"):
        K.weight_table(2, 0)


REFUSALS = [({"src": None}, "null pointer"), ({"out": None}, "null pointer"), ({"weights": None}, "null pointer"),
            ({"fmt": 2}, "fmt 2"), ({"B": 0}, "batch 0"), ({"h": 0}, "a 0x7 plane"), ({"w": 4097}, "a 5x4097 plane"),
            ({"top": 0}, "top 0"), ({"fmt": 0, "top": 300}, "top 300"), ({"radius": 0}, "radius 0 (1..4)"), ({"radius": 5}, "radius 5 (1..4)"),
            ({"passes": 0}, "passes 0 (1..3)"), ({"passes": 4}, "passes 4 (1..3)"), ({"tol_abs": -1}, "tolerance -1"),
            ({"top": 100, "tol_abs": 101}, "tolerance 101"), ({"tol_rel": 65536}, "tolerance_rel 65536"), ({"pairs": 2}, "pairs 2 (0 or 1)"),
            ({"same": True}, "in and out are the same buffer")]


def smooth_caller(lib, src, out, weights, counts=None, ws=None, ws_bytes=0, stream=None):
    """The good call of REFUSALS -- u16 codes, one 5 x 7 plane, the defaults -- over the given addresses, with what a refusal changes
    as keyword arguments; -> (status, message).  Shared with the GPU test"""
    P_ = C.c_void_p
    good = dict(B=1, h=5, w=7, src=src, fmt=1, top=65535, radius=2, passes=2, tol_abs=2, tol_rel=RQ, pairs=1, weights=weights, out=out,
                counts=counts, ws=ws, ws_bytes=ws_bytes)

    def call(same=False, **kw):
        a = dict(good, **kw)
        st = lib.codon_smooth_depth(a["B"], a["h"], a["w"], P_(a["src"]), a["fmt"], a["top"], a["radius"], a["passes"], a["tol_abs"],
                                    a["tol_rel"], a["pairs"], P_(a["weights"]), P_(a["src"] if same else a["out"]), P_(a["counts"]),
                                    P_(a["ws"]), a["ws_bytes"], stream)
        return st, lib.codon_last_error_string().decode()
    return call


def smooth_refusals(lib, call):
    for kw, word in REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and word in msg and msg.startswith("smooth_depth"), (kw, st, msg)


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    call = smooth_caller(lib, 4096, 12288, 20480)                     # never dereferenced: every call is refused on the host
    smooth_refusals(lib, call)
    for kw in ({"src": 4097}, {"out": 12289}, {"counts": 20482}, {"weights": 20482}, {"ws": 40968, "radius": 4, "passes": 3}):
        st, msg = call(**kw)
        assert st == -1 and "unaligned" in msg, (kw, msg)
    if K.plan(4, 3)["launches"] > 1:                                  # the workspace is asked for only where the rule splits the call
        for kw, word in (({}, "null workspace"), ({"ws": 4096}, "the workspace is in or out"), ({"ws": 40960, "ws_bytes": 64}, "too small")):
            st, msg = call(radius=4, passes=3, **kw)
            assert st == -1 and word in msg, (kw, msg)
    q = lib.codon_smooth_workspace_bytes
    assert q(1, 5, 7) == 80 and q(3, 424, 512) == 3 * 424 * 512 * 2 and [q(0, 5, 7), q(1, 0, 7), q(1, 5, 4097), q(65536, 1, 1)] == [0] * 4


NEEDED = ["--depth", "in", "--out", "out"]


@pytest.mark.parametrize("argv, word", [
    (["--radius", "0"], r"--radius 0 \(an integer in 1\.\.4\)"), (["--radius", "5"], r"--radius 5"), (["--passes", "0"], r"--passes 0"),
    (["--passes", "4"], r"--passes 4 \(an integer in 1\.\.3\)"), (["--sigma", "0"], r"--sigma: '0' is not a finite positive number"),
    (["--sigma", "nan"], r"--sigma: 'nan' is not"), (["--sigma", "inf"], r"--sigma: 'inf' is not"), (["--tolerance", "-1"], r"--tolerance -1"),
    (["--tolerance", "256"], r"--tolerance 256 is above the largest code 255"), (["--tolerance-rel", "1.0"], r"--tolerance-rel 1\.0"),
    (["--depth-max", "10000"], r"--depth-max needs --depth-bits 16"),
    (["--depth-bits", "16", "--depth-max", "100", "--tolerance", "101"], r"--tolerance 101 is above the largest code 100"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        K.parse_args(NEEDED + argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_command_line_defaults_and_out_is_depth(capsys):
    a, _, f = K.parse_args(NEEDED)
    assert (a.depth_bits, a.depth_max, a.stats) == (8, None, False)
    assert (f.radius, f.passes, f.sigma, f.tolerance, f.tolerance_rel_q16, f.pairs) == (2, 2, None, 2, RQ, True)
    _, _, f = K.parse_args(NEEDED + ["--radius", "4", "--passes", "3", "--sigma", "0.8", "--tolerance", "7", "--tolerance-rel", "0", "--no-pairs"])
    assert (f.radius, f.passes, f.sigma, f.tolerance, f.tolerance_rel_q16, f.pairs) == (4, 3, 0.8, 7, 0, False)
    with pytest.raises(SystemExit):
        K.parse_args(["--depth", "here", "--out", "./here"])
    assert "--out is --depth" in capsys.readouterr().err


REG = ["--depth", "in", "--calib", "rig.json", "--out", "out"]


@pytest.mark.parametrize("argv, word", [
    (["--smooth-radius", "3"], "--smooth-radius needs --smooth"), (["--smooth-passes", "1"], "--smooth-passes needs --smooth"),
    (["--smooth-sigma", "1.5"], "--smooth-sigma needs --smooth"), (["--smooth-tolerance", "3"], "--smooth-tolerance needs --smooth"),
    (["--smooth-tolerance-rel", "0.1"], "--smooth-tolerance-rel needs --smooth"), (["--smooth-no-pairs"], "--smooth-no-pairs needs --smooth"),
    (["--smooth", "--smooth-radius", "5"], r"--smooth-radius 5 \(an integer in 1\.\.4\)"),
    (["--smooth", "--smooth-tolerance", "256"], "--smooth-tolerance 256 is above the largest code 255"),
])
def test_register_refuses_by_name(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        P.parse_args(REG + argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_register_without_smooth_builds_no_smoother():
    a, _ = P.parse_args(REG)
    assert a.smoother is None and a.cleaner is None
    a, _ = P.parse_args(REG + ["--smooth", "--smooth-no-pairs", "--smooth-passes", "3"])
    assert (a.smoother.passes, a.smoother.pairs, a.smoother.radius) == (3, False, 2)
