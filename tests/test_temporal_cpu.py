"""The temporal filter's definition (tests/temporal_ref.py) on the CPU: what the definition promises -- the identity
for a window of one frame and for equal frames, symmetry under time reversal and under any permutation of the pixels, outputs
inside the window's range and within tau of an accepted input -- the median's rank, the two sides of the link, the clamps at the
sequence's ends, the committed scene's assertions on all three grids, and every refusal that needs no GPU: of TemporalFilter, of
the C entry (validated on the host before any HIP call) and of the command line.  Expectations are spelled out here, not derived
from the code under test."""
import ctypes as C
import re

import numpy as np
import pytest

from codon_amd import _lib as L
from codon_amd import temporal as K
from tests import clean_ref
from tests import temporal_ref as R

RQ = 1311                                   # rint(65536 * 0.02)
FORMATS = ((np.uint8, 255), (np.uint16, 65535), (np.uint16, 10000))
IDS = ["u8", "u16", "u16_10000"]


def _random(T, h, w, top, dtype, seed):
    """A static level per pixel under +- 2 codes of noise, 30 % holes, one sample in ten on another level"""
    g = np.random.default_rng(seed)
    levels = np.array([top // 5, top // 2, top - 3])
    c = levels[g.integers(0, 3, size=(h, w))][None] + g.integers(-2, 3, size=(T, h, w))
    c = np.where(g.random((T, h, w)) < 0.1, levels[g.integers(0, 3, size=(T, h, w))], c)
    c[g.random((T, h, w)) < 0.3] = 0
    return c.astype(dtype)


def _seq(*codes):
    """One pixel through time"""
    return np.array(codes, dtype=np.uint16).reshape(-1, 1, 1)


def _one(codes, t, back, ahead, A=2, Rq=RQ, M=2, F=2):
    return int(R.temporal(_seq(*codes), back, ahead, A, Rq, M, F)[0][t, 0, 0])


def test_the_defaults_and_the_names():
    assert R.DEFAULTS == K.DEFAULTS == dict(window=5, causal=False, tolerance=2, tolerance_rel=0.02, min_count=2, min_fill=2)
    assert R.STATS == K.STATS == ("valid", "rejected", "filled", "changed")
    assert (R.MAX_WINDOW, R.MAX_FRAMES) == (K.MAX_WINDOW, K.MAX_FRAMES) == (15, 4096)
    f = K.TemporalFilter()
    assert (f.back, f.ahead, f.window, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (2, 2, 5, 2, RQ, 2, 2)
    assert (K.TemporalFilter(window=4, causal=True).back, K.TemporalFilter(window=4, causal=True).ahead) == (3, 0)
    f = K.TemporalFilter(back=2, ahead=5)
    assert (f.back, f.ahead, f.window) == (2, 5, 8)
    f = K.TemporalFilter(15, False, 65535, 65535 / 65536, 15, 15)
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (7, 7, 65535, 65535, 15, 15)
    f = K.TemporalFilter(1, True, 0, 0.0, 1, 0)
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (0, 0, 0, 0, 1, 0)
    assert (K.TemporalFilter(back=14, ahead=0).window, K.TemporalFilter(back=0, ahead=14).window) == (15, 15)


def test_the_link_function_is_cleans():
    g = np.random.default_rng(7)
    a, b = g.integers(0, 65536, size=20000), g.integers(0, 65536, size=20000)
    b[::3] = np.clip(a[::3] + g.integers(-900, 901, size=a[::3].size), 0, 65535)            # many pairs near tau
    for A, Rq in ((2, RQ), (0, RQ), (8, 0), (0, 0), (65535, 65535)):
        want = clean_ref.linked(a, b, A, Rq)
        assert np.array_equal(R.linked(a, b, A, Rq), want) and 0 < want.sum() <= a.size
    assert R.rel_q16(0.02) == clean_ref.rel_q16(0.02) == RQ == K.rel_q16("t", 0.02)


@pytest.mark.parametrize("v", [10, 40000])
def test_the_link_holds_at_tau_and_not_one_beyond(v):
    """A = 2, Rq = 1311: tau(10) = 2 + (13110 >> 16) = 2, tau(40000) = 2 + (52440000 >> 16) = 2 + 800.  Two frames, M = 2, F = 0: a
    linked pair is its rounded mean in both frames, an unlinked pair is rejected twice"""
    tau = {10: 2, 40000: 802}[v]
    for d, want in ((tau, True), (tau + 1, False)):
        assert bool(R.linked(np.array([v]), np.array([v + d]), 2, RQ)[0]) is want
        out, stats = R.temporal(_seq(v, v + d), 1, 1, 2, RQ, 2, 0)
        mean = (2 * (2 * v + d) + 2) // 4
        assert out.ravel().tolist() == ([mean, mean] if want else [0, 0])
        assert stats.tolist() == ([[1, 0, 0, 1]] * 2 if want else [[1, 1, 0, 0]] * 2)


@pytest.mark.parametrize("dtype, top", FORMATS, ids=IDS)
def test_a_window_of_one_frame_and_equal_frames_are_the_identity(dtype, top):
    c = _random(6, 9, 11, top, dtype, 3)
    for M, F in ((1, 0), (2, 2), (15, 15)):
        out, stats = R.temporal(c, 0, 0, 2, RQ, M, F)
        assert out.dtype == c.dtype and out.tobytes() == c.tobytes()
        assert stats.tolist() == [[int((p != 0).sum()), 0, 0, 0] for p in c]
    same = np.repeat(c[:1], 7, axis=0)
    for Bk, Ah in ((1, 1), (7, 7), (14, 0), (0, 14), (2, 5)):
        out, stats = R.temporal(same, Bk, Ah, 2, RQ, 2, 2)
        assert out.tobytes() == same.tobytes() and not stats[:, 1:].any()


@pytest.mark.parametrize("dtype, top", FORMATS, ids=IDS)
def test_time_reversal_and_pixel_permutations_commute(dtype, top):
    c = _random(19, 7, 5, top, dtype, 4)
    g = np.random.default_rng(5)
    perm = g.permutation(35)
    for Bk, Ah, M, F in ((2, 2, 2, 2), (5, 1, 3, 2), (0, 14, 2, 4), (3, 0, 1, 3)):
        out, stats = R.temporal(c, Bk, Ah, 1, RQ, M, F)
        assert stats[:, 1].sum() > 0 or M == 1
        assert stats[:, 2].sum() > 0
        rev, rstats = R.temporal(np.ascontiguousarray(c[::-1]), Ah, Bk, 1, RQ, M, F)
        assert np.array_equal(rev[::-1], out) and np.array_equal(rstats[::-1], stats)
        mixed = c.reshape(19, 35)[:, perm].reshape(19, 5, 7)
        pout, pstats = R.temporal(mixed, Bk, Ah, 1, RQ, M, F)
        assert np.array_equal(pout.reshape(19, 35), out.reshape(19, 35)[:, perm]) and np.array_equal(pstats, stats)


@pytest.mark.parametrize("dtype, top", FORMATS, ids=IDS)
def test_outputs_lie_in_the_windows_range_and_within_tau_of_an_accepted_input(dtype, top):
    c = _random(23, 6, 8, top, dtype, 6)
    x = c.astype(np.int64)
    for Bk, Ah, A, M, F in ((2, 2, 2, 2, 2), (7, 7, 0, 3, 1), (0, 4, 5, 1, 0), (14, 0, 2, 15, 15)):
        out, stats, rej = R.temporal(c, Bk, Ah, A, RQ, M, F, details=True)
        o = out.astype(np.int64)
        for t in range(23):
            lo, hi = R.window_of(t, 23, Bk, Ah)
            S = x[lo:hi + 1]
            big = np.where(S != 0, S, 1 << 40).min(axis=0)
            nz = o[t] != 0
            assert (o[t][nz] >= big[nz]).all() and (o[t][nz] <= S.max(axis=0)[nz]).all() and o[t].max() <= top
        kept = (x != 0) & ~rej
        assert (o[kept] != 0).all() and (np.abs(o - x)[kept] <= A + ((RQ * x[kept]) >> 16)).all()
        if M == 1 and F == 0:               # holes stay holes and valid pixels stay valid
            assert np.array_equal(o != 0, x != 0) and not stats[:, 1:3].any()


def test_the_medians_rank_on_even_and_odd_counts_with_ties():
    S = lambda *v: np.array(v, dtype=np.int64).reshape(-1, 1)                   # noqa: E731
    for samples, want in (((5,), 5), ((9, 5), 5), ((9, 5, 7), 7), ((9, 5, 7, 0, 3), 5), ((4, 4, 9, 9), 4), ((9, 4, 9, 4, 9), 9),
                          ((0, 0, 0), 0), ((0, 8, 0), 8), ((7, 7, 7, 7), 7), ((1, 2, 3, 4, 5, 6), 3), ((6, 5, 4, 3, 2, 1, 0), 3)):
        m, k = R.lower_median(S(*samples))
        assert int(m[0]) == want and int(k[0]) == sum(s != 0 for s in samples), samples
    # through the filter: a hole among 100, 100, 500, 500 takes the LOWER pair (rank 1 of 4), among 100, 500, 500 the upper
    assert _one((100, 100, 0, 500, 500), 2, 2, 2) == 100
    assert _one((100, 0, 500, 500), 1, 1, 2) == 500
    assert _one((100, 0, 500), 1, 1, 1) == 0                   # the median 100 has one linked sample: below F = 2


def test_the_clamps_at_the_sequence_ends():
    """M is clamped by the frames of the window, F is not"""
    c = np.array([[[700, 0, 41]]], dtype=np.uint16)
    out, stats = R.temporal(c, 2, 2, 2, RQ, 2, 2)
    assert out.tobytes() == c.tobytes() and stats.tolist() == [[2, 0, 0, 0]]            # T = 1, M = 2: min(M, 1) = 1
    assert _one((700, 900), 0, 0, 1, M=2, F=0) == 0           # two frames: the clamp is 2, and 700 stands alone
    assert _one((700, 900), 0, 0, 0, M=2, F=0) == 700         # ... but in a window of itself it does not
    assert _one((0, 700), 0, 0, 1, F=1) == 700 and _one((0, 700), 0, 0, 1, F=2) == 0            # F = 2 needs two samples, n_w or not
    assert _one((0, 700, 701), 0, 0, 2, F=3) == 0 and _one((0, 700, 701), 0, 0, 2, F=2) == 701           # (1401 * 2 + 2) // 4 = 701


def test_a_rejected_spike_takes_the_consensus_or_becomes_a_hole():
    codes = (1000, 1001, 5000, 999, 1000)
    out, stats = R.temporal(_seq(*codes), 2, 2, 2, RQ, 2, 2)
    # frame 0 sees 1000, 1001 and the spike: 1000.5 rounds up; the spike takes the mean of the four others, linked to the median 1000
    assert out.ravel().tolist() == [1001, 1000, 1000, 1000, 1000]
    assert stats[2].tolist() == [1, 1, 1, 0] and stats[:, 1].sum() == 1
    out, stats = R.temporal(_seq(*codes), 2, 2, 2, RQ, 2, 0)
    assert out.ravel().tolist() == [1001, 1000, 0, 1000, 1000] and stats[2].tolist() == [1, 1, 0, 0]
    out, stats = R.temporal(_seq(*codes), 2, 2, 2, RQ, 1, 0)                                # rejection off: the spike stays
    assert out.ravel().tolist() == [1001, 1000, 5000, 1000, 1000] and not stats[:, 1].any()
    # a moving occlusion edge: the near surface arrives at frame 3; no output lies between the two surfaces
    out, _ = R.temporal(_seq(3000, 3001, 2999, 1000, 1001, 1000), 2, 2, 2, RQ, 2, 2)
    assert out.ravel().tolist() == [3000, 3000, 3000, 1000, 1000, 1000]


@pytest.mark.parametrize("top", [10000, 65535, 255])
def test_the_scene(top):
    """The committed scene under the defaults (window 5, M = 2, F = 2; A scaled with the grid), on all three grids: every spike is
    rejected, every flicker hole outside the band and away from the rectangle's path is filled, the band stays empty, no output
    lies strictly between the two surfaces, and the mean absolute error against the noiseless frames falls"""
    c, flicker, spikes = R.scene(top)
    assert c.shape == (16, 40, 100) and flicker.sum() == 600 and spikes.sum() == 60 and not (flicker & spikes).any()
    assert (c[flicker] == 0).all() and (c[spikes] != 0).all() and not c[:, 34:37].any()
    assert ((c == 0).sum(axis=0)[:34] <= 1).all()                        # one event per pixel: a flicker hole stands alone in time
    out, stats, rej = R.temporal(c, 2, 2, R.SCENE_TOLERANCE[top], RQ, 2, 2, details=True)
    o, x, truth = out.astype(np.int64), c.astype(np.int64), R.scene_truth(top)
    assert rej[spikes].all() and int(rej.sum()) == 60 == int(stats[:, 1].sum())
    away = flicker & ~R.path_mask()[None]
    assert away.sum() > 200 and (o[away] != 0).all()
    assert int(stats[:, 2].sum()) == 660 and (o[flicker] != 0).all() and (o[spikes] != 0).all()
    assert not o[:, 34:37].any()
    lo, hi = int(np.rint(R.NEAR_HI * top / 10000)), int(np.rint(R.FAR_LO * top / 10000))
    assert not ((o > lo) & (o < hi)).any() and not ((x > lo) & (x < hi)).any()
    both = (x != 0) & (o != 0)
    before, after = np.abs(x - truth)[both].mean(), np.abs(o - truth)[both].mean()
    print(f"top {top}: mean absolute error against the noiseless frames {before:.4f} codes before, {after:.4f} after")
    assert after < before
    calm = both & ~spikes                                                # and without the spikes' share of it: the range noise alone
    print(f"top {top}: without the spikes {np.abs(x - truth)[calm].mean():.4f} before, {np.abs(o - truth)[calm].mean():.4f} after")


def test_the_chunk_rule_is_the_librarys():
    """tests/temporal_ref.chunk_frames restates csrc/launch_rules.h; the library's own answer, asked without a launch"""
    q = L.load().codon_temporal_chunk_frames
    for T in (1, 7, 8, 9, 17, 56, 57, 64, 1000, 4096):
        for h, w in ((1, 1), (5, 7), (40, 100), (424, 512), (480, 640)):
            for Bk, Ah in R.WINDOWS:
                assert q(T, h, w, Bk, Ah) == R.chunk_frames(T, h, w, Bk, Ah), (T, h, w, Bk, Ah)
    assert q(64, 424, 512, 2, 2) == 13 and q(64, 424, 512, 7, 7) == 28 and q(4096, 1, 1, 0, 0) == 8 and q(7, 1, 1, 0, 0) == 7
    assert q(0, 5, 7, 2, 2) == 0 and q(3, 5, 7, 8, 7) == 0 and q(128, 4096, 4096, 2, 2) == 0 and q(3, 0, 7, 2, 2) == 0
    assert (R.TILE, R.PER) == (1024, 4)


def test_what_the_case_set_covers():
    """From the restatement: some case rejects, some fills, some does both in one call, some window straddles a chunk seam; every
    window register count is taken; codes of 32768 and above occur; whole quads and partial ones"""
    rows = R.cases()
    assert len(rows) == len(set(rows)) == 427
    rejects = fills = both = seams = 0
    for case in rows:
        T, h, w, Bk, Ah = case[:5]
        _, stats = R.want(case)
        r, f = int(stats[:, 1].sum()) > 0, int(stats[:, 2].sum()) > 0
        rejects, fills, both = rejects + r, fills + f, both + (r and f)
        seams += Bk + Ah > 0 and R.chunk_frames(T, h, w, Bk, Ah) < T
    assert rejects > 50 and fills > 50 and both > 30 and seams > 50
    assert {Bk + Ah + 1 for Bk, Ah in R.WINDOWS} == {1, 3, 5, 8, 15}
    assert {(h * w) % R.PER == 0 for _, h, w, *_ in rows} == {True, False} and any(w % R.PER == 1 and w > R.PER for _, _, w, *_ in rows)
    assert any(R.sequence(c[0], c[1], c[2], "high", 65535).max() == 65535 for c in rows if c[9] == "high")
    single = R.sequence(17, 5, 7, "single", 10000)
    assert ((single != 0).sum(axis=0) == 1).all()


# ---- the refusals -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kw, word", [
    (dict(window=0), "window 0 "), (dict(window=16), "window 16 "), (dict(window=4), "window 4 "), (dict(window=5.0), "window 5.0 "),
    (dict(window=True), "window True "), (dict(window=16, causal=True), "window 16 "), (dict(causal=1), "causal 1 "),
    (dict(back=-1, ahead=0), "back -1 "), (dict(back=8, ahead=7), "ahead 7 "), (dict(back=2), "ahead None "),
    (dict(ahead=2), "back None "), (dict(back=15, ahead=0), "back 15 "), (dict(back=1.0, ahead=1), "back 1.0 "),
    (dict(tolerance=-1), "tolerance -1 "), (dict(tolerance=65536), "tolerance 65536 "), (dict(tolerance=2.0), "tolerance 2.0 "),
    (dict(tolerance_rel=-0.01), "tolerance_rel -0.01 "), (dict(tolerance_rel=1.0), "tolerance_rel 1.0 "),
    (dict(tolerance_rel=float("nan")), "tolerance_rel nan "), (dict(tolerance_rel="x"), "tolerance_rel 'x' "),
    (dict(min_count=0), "min_count 0 "), (dict(min_count=16), "min_count 16 "), (dict(min_count=2.0), "min_count 2.0 "),
    (dict(min_fill=-1), "min_fill -1 "), (dict(min_fill=16), "min_fill 16 "), (dict(min_fill=None), "min_fill None "),
])
def test_filter_refusals(kw, word):
    with pytest.raises(ValueError, match="TemporalFilter: " + re.escape(word)):
        K.TemporalFilter(**kw)


def temporal_refusals(lib, call):
    """call(**what differs) -> (status, message) of codon_temporal_depth; shared with the GPU test"""
    for kw, word in R.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("temporal_depth: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="temporal_depth failed with status -1: temporal_depth: "):
            L.check(st, "temporal_depth")


def temporal_caller(lib, src, out, counts=None, stream=None):
    """The good call of temporal_ref.REFUSALS -- u16 codes, three 5 x 7 frames, the defaults -- over the given addresses, with what
    a refusal changes as keyword arguments"""
    P_ = C.c_void_p

    def call(T=3, h=5, w=7, src=src, fmt=L.FILL_U16, top=65535, back=2, ahead=2, tol_abs=2, tol_rel=RQ, count=2, fill=2, out=out,
             counts=counts):
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_temporal_depth(T, h, w, p(src), fmt, top, back, ahead, tol_abs, tol_rel, count, fill, p(out), p(counts), stream)
        return st, lib.codon_last_error_string().decode()
    return call


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    call = temporal_caller(lib, 4096, 12288)                        # never dereferenced: every call is refused on the host
    temporal_refusals(lib, call)
    for kw in ({"src": 4097}, {"out": 12289}, {"counts": 20482}):
        assert "unaligned" in call(**kw)[1], kw
    # of two broken rules the first in the argument list is reported
    assert "frames 0 " in call(T=0, fmt=5)[1] and "fmt 5 " in call(fmt=5, top=0)[1] and "window" in call(back=-1, count=0)[1]
    assert "min_count 0 " in call(count=0, fill=16)[1] and "min_fill 16 " in call(fill=16, out="src")[1]
    # at the bounds themselves the refusal is the alias asked for beside them: no bound is off by one
    at = dict(T=4096, h=1, w=4096, top=10000, tol_abs=10000, tol_rel=65535, count=15, fill=15, out="src")
    assert "same buffer" in call(back=14, ahead=0, **at)[1] and "same buffer" in call(back=0, ahead=14, **at)[1]
    assert "same buffer" in call(T=127, h=4096, w=4096, tol_abs=0, tol_rel=0, count=1, fill=0, back=0, ahead=0, out="src")[1]


NEEDED = ["--depth", "d", "--out", "o"]


@pytest.mark.parametrize("argv, word", [
    (["--out", "o"], "the following arguments are required: --depth"),
    (["--depth", "d"], "the following arguments are required: --out"),
    ([*NEEDED, "--depth-bits", "12"], "invalid choice"),
    ([*NEEDED, "--depth-max", "10000"], "--depth-max needs --depth-bits 16"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "0"], "--depth-max 0 must be in \\[1, 65535\\]"),
    (["--depth", "d", "--out", "./d"], "--out is --depth"),
    ([*NEEDED, "--window", "0"], "--window 0 "),
    ([*NEEDED, "--window", "4"], "--window 4 "),
    ([*NEEDED, "--window", "16", "--causal"], "--window 16 "),
    ([*NEEDED, "--window", "17"], "--window 17 "),
    ([*NEEDED, "--window", "5.5"], "invalid int value"),
    ([*NEEDED, "--tolerance", "-1"], "--tolerance -1 "),
    ([*NEEDED, "--tolerance", "256"], "--tolerance 256 is above the largest code 255"),
    ([*NEEDED, "--depth-bits", "16", "--depth-max", "10000", "--tolerance", "10001"], "--tolerance 10001 is above the largest code 10000"),
    ([*NEEDED, "--tolerance-rel", "1.0"], "--tolerance-rel 1.0 "),
    ([*NEEDED, "--tolerance-rel", "nan"], "--tolerance-rel nan "),
    ([*NEEDED, "--min-count", "0"], "--min-count 0 "),
    ([*NEEDED, "--min-count", "16"], "--min-count 16 "),
    ([*NEEDED, "--min-fill", "-1"], "--min-fill -1 "),
    ([*NEEDED, "--min-fill", "16"], "--min-fill 16 "),
    ([*NEEDED, "--block", "0"], "--block 0 must be in"),
    ([*NEEDED, "--block", "4083"], "--block 4083 must be in"),
])
def test_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        K.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_command_line_defaults_and_blocks(tmp_path, capsys):
    a, _, f = K.parse_args(NEEDED)
    assert (a.depth_bits, a.depth_max, a.window, a.causal, a.block, a.stats) == (8, None, 5, False, 256, False)
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (2, 2, 2, RQ, 2, 2)
    a, _, f = K.parse_args([*NEEDED, "--depth-bits", "16", "--depth-max", "10000", "--window", "6", "--causal", "--tolerance", "8",
                            "--tolerance-rel", "0.05", "--min-count", "3", "--min-fill", "0", "--block", "4", "--stats"])
    assert (a.depth_bits, a.depth_max, a.block, a.stats) == (16, 10000, 4, True)
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (5, 0, 8, 3277, 3, 0)
    with pytest.raises(SystemExit) as e:                                 # the directory is looked at before the GPU is asked for
        K.main(["--depth", str(tmp_path / "none"), "--out", str(tmp_path / "o")])
    assert e.value.code == 2 and "is not a directory" in capsys.readouterr().err
    # every frame is written by exactly one block, from an upload that holds its whole window
    assert K.blocks(10, 4, 2, 1) == [(0, 4, 0, 5), (4, 8, 2, 9), (8, 10, 6, 10)]
    assert K.blocks(3, 256, 7, 7) == [(0, 3, 0, 3)] and K.blocks(0, 4, 2, 2) == []
    for n, block, Bk, Ah in ((17, 4, 2, 2), (9, 1, 14, 0), (30, 7, 0, 14)):
        c = _random(n, 3, 4, 10000, np.uint16, n)
        whole, wstats = R.temporal(c, Bk, Ah, 2, RQ, 2, 2)
        for first, stop, lo, hi in K.blocks(n, block, Bk, Ah):
            part, pstats = R.temporal(c[lo:hi], Bk, Ah, 2, RQ, 2, 2)
            assert np.array_equal(part[first - lo:stop - lo], whole[first:stop])
            assert np.array_equal(pstats[first - lo:stop - lo], wstats[first:stop])
