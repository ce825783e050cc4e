"""The temporal stream (codon_amd.temporal.TemporalStream, codon_temporal_push) without a GPU: the premise of its
ring of 16 slots, walked in pure Python for every window and length; the order and count of what a stream emits; every refusal of
TemporalStream, of the C entry (validated on the host before any HIP call: the addresses are never dereferenced) and of the two
command lines; the library's ring size; and that temporal.parse_args still yields what it yielded.  Expectations are spelled out
here, not derived from the code under test."""
import ctypes as C
import re

import pytest
import torch

from codon_amd import _lib as L
from codon_amd import register as P
from codon_amd import temporal as K
from tests import temporal_ref as R
from tests import temporal_stream_cases as S

RQ = 1311                                   # rint(65536 * 0.02)
SLOTS = 16


def _walk(T, back, ahead, slots=SLOTS):
    """The stream's rule, restated: frame s goes into slot s & 15.  A push step with N frames in emits t = N - 1 - ahead if
    t >= 0; flush step F emits t = max(0, N - ahead) + F - 1 if t <= N - 1; either reads frames max(0, t - back) .. N - 1.
    -> [(frame, step)] emitted; asserts that every slot read still holds the frame the window means"""
    slot = [None] * slots
    out = []

    def emit(t, N, step):
        lo, hi = max(0, t - back), N - 1
        assert hi == min(N - 1, t + ahead) and hi - lo + 1 <= back + ahead + 1 <= 15
        assert (lo, hi) == R.window_of(t, T, back, ahead)           # the definition's window of the WHOLE sequence
        for f in range(lo, hi + 1):
            assert slot[f & (slots - 1)] == f, (T, back, ahead, t, f, slot)
        out.append((t, step))

    for s in range(T):
        slot[s & (slots - 1)] = s
        N = s + 1
        if N - 1 - ahead >= 0:
            emit(N - 1 - ahead, N, s)
    for F in range(1, ahead + 2):            # one flush step more than any stream owes
        t = max(0, T - ahead) + F - 1
        if t <= T - 1:
            emit(t, T, T + F - 1)
    return out


def test_sixteen_slots_hold_every_frame_a_pending_window_reads():
    """For every (back, ahead) with back + ahead <= 14 and every T <= 40: no slot a window reads has been overwritten, pushes and
    flush included; every frame is emitted once, in order; a flushed frame's window is the definition's at the sequence's end"""
    windows = 0
    for back in range(15):
        for ahead in range(15 - back):
            windows += 1
            for T in range(0, 41):
                got = _walk(T, back, ahead)
                assert [t for t, _ in got] == list(range(T))
                assert got == S.emitted_by(T, ahead)
    assert windows == 120
    # the arithmetic of the header: storing frame N - 1 overwrites N - 17; the oldest frame still read is N - 1 - ahead - back >= N - 15
    assert all(n - 1 - a - b >= n - 15 > n - 17 for n in (17, 100) for b in range(15) for a in range(15 - b))
    # and the walk is no formality: eight slots do not hold a window of fifteen
    with pytest.raises(AssertionError):
        _walk(20, 7, 7, slots=8)


def test_the_order_and_count_of_every_case():
    """T outputs for T inputs; frame t is the answer of push t + ahead, or of the flush when fewer than ahead frames follow it"""
    rows = S.cases()
    assert len(rows) == len(set(rows)) == 309
    assert {Bk + Ah + 1 for _, _, _, Bk, Ah, *_ in rows} == {1, 3, 5, 8, 15}
    assert {T for T, *_ in rows} >= {1, 2, 15, 16, 17, 33} and {c[1:3] for c in rows} == set(R.PLANES)
    assert {c[0] for c in rows if c[1:3] == R.BIG_PLANE} == {1, 3, 17}
    assert any(T <= Ah for T, _, _, _, Ah, *_ in rows) and {c[10] for c in rows} == {255, 65535, 10000}
    for T, h, w, Bk, Ah, *_ in rows:
        got = S.emitted_by(T, Ah)
        assert got == _walk(T, Bk, Ah) and len(got) == T
        pushes = [t for t, step in got if step < T]
        assert pushes == list(range(max(0, T - Ah))) and all(step == t + Ah for t, step in got if step < T)
        assert [step for t, step in got if step >= T] == list(range(T, T + min(Ah, T)))
    assert S.emitted_by(3, 2) == [(0, 2), (1, 3), (2, 4)] and S.emitted_by(2, 5) == [(0, 2), (1, 3)] and S.emitted_by(2, 0) == [(0, 0), (1, 1)]


# ---- the C entry --------------------------------------------------------------------------------------------------------------------

def push_caller(lib, src=4096, ring=65536, state=8192, out=12288, counts=None, stream=None):
    """The good call -- u16 codes, a 5 x 7 frame, the defaults -- over the given addresses (a plane is 70 bytes, the ring 1120), with
    what a refusal changes as keyword arguments; shared with the GPU test"""
    P_ = C.c_void_p

    def call(h=5, w=7, src=src, fmt=L.FILL_U16, top=65535, back=2, ahead=2, tol_abs=2, tol_rel=RQ, count=2, fill=2, ring=ring,
             state=state, out=out, counts=counts):
        out = src if out == "src" else out
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_temporal_push(h, w, p(src), fmt, top, back, ahead, tol_abs, tol_rel, count, fill, p(ring), p(state), p(out),
                                     p(counts), stream)
        return st, lib.codon_last_error_string().decode()
    return call


# (what differs from the good call, a piece of the message), in the order the entry checks them; ring addresses are relative to the
# caller's src (S) and out (O): a ring is 16 planes of 70 bytes
def push_refusals(src, out):
    return [({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"), ({"h": 4097}, "a 4097x7 plane"), ({"w": 4097}, "a 5x4097 plane"),
            ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "),
            ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "), ({"fmt": 0, "top": 1000}, "top 1000 "),
            ({"back": -1}, "window back -1 ahead 2"), ({"ahead": -1}, "window back 2 ahead -1"), ({"back": 8, "ahead": 7}, "window back 8 ahead 7"),
            ({"back": 15, "ahead": 0}, "window back 15 ahead 0"),
            ({"tol_abs": -1}, "tolerance -1 "), ({"top": 10000, "tol_abs": 10001}, "tolerance 10001 "),
            ({"tol_rel": -1}, "tolerance_rel -1 "), ({"tol_rel": 65536}, "tolerance_rel 65536 "),
            ({"count": 0}, "min_count 0 "), ({"count": 16}, "min_count 16 "),
            ({"fill": -1}, "min_fill -1 "), ({"fill": 16}, "min_fill 16 "),
            ({"ring": None}, "null pointer"), ({"state": None}, "null pointer"), ({"out": None}, "null pointer"),
            ({"out": "src"}, "same buffer"),
            ({"ring": src}, "the ring overlaps in"), ({"ring": src + 68}, "the ring overlaps in"), ({"ring": src - 1120 + 2}, "the ring overlaps in"),
            ({"ring": out}, "the ring overlaps out"), ({"ring": out + 68}, "the ring overlaps out"), ({"ring": out - 1120 + 2}, "the ring overlaps out"),
            ({"src": None, "ring": out - 560}, "the ring overlaps out")]


def check_push_refusals(lib, call, src, out):
    for kw, word in push_refusals(src, out):
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("temporal_push: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="temporal_push failed with status -1: temporal_push: "):
            L.check(st, "temporal_push")


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    call = push_caller(lib)                                          # never dereferenced: every call here is refused on the host
    check_push_refusals(lib, call, 4096, 12288)
    for kw in ({"src": 4097}, {"out": 12289}, {"ring": 65537}, {"state": 8194}, {"state": 8193}, {"counts": 20482}):
        assert "unaligned" in call(**kw)[1], kw
    # of two broken rules the first in the argument list is reported
    assert "a 0x7 plane" in call(h=0, fmt=5)[1] and "fmt 5 " in call(fmt=5, top=0)[1] and "top 0 " in call(top=0, back=-1)[1]
    assert "window" in call(back=-1, tol_abs=-1)[1] and "tolerance -1 " in call(tol_abs=-1, tol_rel=-1)[1]
    assert "tolerance_rel -1 " in call(tol_rel=-1, count=0)[1] and "min_count 0 " in call(count=0, fill=16)[1]
    assert "min_fill 16 " in call(fill=16, ring=None)[1] and "null pointer" in call(state=None, out="src")[1]
    assert "same buffer" in call(out="src", ring=4096)[1] and "overlaps in" in call(ring=4096 + 2, state=8193)[1]
    # at the bounds themselves the refusal is the last rule's, asked for beside them: no bound is off by one.  A ring that ends where
    # `in` begins, or begins where `out` ends, overlaps neither; a flush step has no `in`
    at = dict(top=10000, tol_abs=10000, tol_rel=65535, count=15, fill=15, state=8194)
    assert "unaligned" in call(h=1, w=4096, back=14, ahead=0, **at)[1] and "unaligned" in call(h=4096, w=1, back=0, ahead=14, **at)[1]
    assert "unaligned" in call(h=4096, w=4096, ring=1 << 40, tol_abs=0, tol_rel=0, count=1, fill=0, back=0, ahead=0, state=8194)[1]
    assert "unaligned" in call(ring=4096 - 1120, state=8194)[1] and "unaligned" in call(ring=4096 + 70, out=1 << 20, state=8194)[1]
    assert "unaligned" in call(ring=12288 + 70, state=8194)[1] and "unaligned" in call(ring=12288 - 1120, src=1 << 20, state=8194)[1]
    assert "unaligned" in call(src=None, state=8194)[1] and "unaligned" in call(src=None, ring=4096, state=8194)[1]
    assert "unaligned" in call(fmt=0, top=255, src=4097, out=12289, ring=65537, state=8194)[1]      # u8 planes stand anywhere
    assert lib.codon_temporal_ring_frames() == SLOTS == 16


# ---- TemporalStream ------------------------------------------------------------------------------------------------------------------

def test_stream_constructor_refusals_and_mirrors():
    f = K.TemporalFilter(back=2, ahead=5)
    s = K.TemporalStream(f, (5, 7), torch.int16, depth_max=10000)
    assert (s.shape, s.dtype, s.top, s.latency, s.frames, s.emitted, s.closed) == ((5, 7), torch.int16, 10000, 5, 0, 0, False)
    assert s.device == torch.device("cuda:0") and K.TemporalStream(f, (1, 4096), torch.uint8).top == 255
    assert K.TemporalStream(f, [4096, 1], torch.uint16, device="cuda:1").device == torch.device("cuda", 1)
    assert K.TemporalStream(K.TemporalFilter(tolerance=255), (5, 7), torch.uint8, depth_max=255).top == 255
    assert K.TemporalStream(K.TemporalFilter(tolerance=10000), (5, 7), torch.uint16, depth_max=10000).top == 10000
    for args, kw, word in [
        (("x", (5, 7), torch.uint8), {}, "filt 'x' "), ((f, 5, torch.uint8), {}, "shape 5 "), ((f, (5,), torch.uint8), {}, "shape (5,) "),
        ((f, (0, 7), torch.uint8), {}, "shape 0 "), ((f, (5, 4097), torch.uint8), {}, "shape 4097 "), ((f, (5.0, 7), torch.uint8), {}, "shape 5.0 "),
        ((f, (5, 7), torch.float32), {}, "dtype torch.float32 "), ((f, (5, 7), torch.uint8), {"depth_max": 1000}, "depth_max 1000 with 8-bit codes"),
        ((f, (5, 7), torch.int16), {"depth_max": 0}, "depth_max 0 must be"), ((f, (5, 7), torch.int16), {"depth_max": 65536}, "depth_max 65536 must be"),
        ((K.TemporalFilter(tolerance=256), (5, 7), torch.uint8), {}, "tolerance 256 above the largest code 255"),
        ((K.TemporalFilter(tolerance=10001), (5, 7), torch.int16), {"depth_max": 10000}, "tolerance 10001 above the largest code 10000"),
        ((f, (5, 7), torch.uint8), {"device": "cpu"}, "device 'cpu' "), ((f, (5, 7), torch.uint8), {"device": "cuda"}, "device 'cuda' "),
    ]:
        with pytest.raises(ValueError, match=re.escape(word)):
            K.TemporalStream(*args, **kw)


def test_stream_push_refusals_without_gpu():
    """A frame of another shape, dtype or device than the stream's, an `out` of the wrong shape or dtype, a push after flush():
    each by name, before anything is allocated or launched"""
    s = K.TemporalStream(K.TemporalFilter(), (5, 7), torch.int16, depth_max=10000)
    good = torch.zeros((5, 7), dtype=torch.int16)
    for frame, kw, exc, word in [
        (torch.zeros((5, 7)), {}, RuntimeError, "temporal_push expects (h,w) uint8 codes"),
        (torch.zeros((5, 7, 1, 1), dtype=torch.int16), {}, RuntimeError, "temporal_push expects"),
        (torch.zeros((7, 5), dtype=torch.int16), {}, ValueError, "temporal_push: a frame of shape (7, 5), the stream's is (5, 7)"),
        (torch.zeros((1, 5, 7), dtype=torch.int16), {}, ValueError, "a frame of shape (1, 5, 7)"),
        (torch.zeros((5, 7), dtype=torch.uint16), {}, ValueError, "temporal_push: a frame of torch.uint16, the stream's is torch.int16"),
        (torch.zeros((5, 7), dtype=torch.uint8), {}, ValueError, "depth_max 10000 with 8-bit codes"),
        (good, {"out": torch.zeros((5, 8), dtype=torch.int16)}, ValueError, "temporal_push: out of shape (5, 8), the stream's is (5, 7)"),
        (good, {"out": torch.zeros((5, 7), dtype=torch.uint8)}, ValueError, "temporal_push: out of torch.uint8, the stream's is torch.int16"),
        (good, {"out": torch.zeros((5, 14), dtype=torch.int16)[:, ::2]}, ValueError, "temporal_push: out is not contiguous"),
        (good, {}, RuntimeError, "temporal_push: a frame on cpu, the stream on cuda:0"),
        (good, {"out": torch.zeros((5, 7), dtype=torch.int16)}, RuntimeError, "temporal_push: a frame on cpu, the stream on cuda:0"),
    ]:
        with pytest.raises(exc, match=re.escape(word)):
            s.push(frame, **kw)
    assert (s.frames, s.emitted, s.closed) == (0, 0, False)
    with pytest.raises(ValueError, match="temporal_push: n -1 "):
        s.replayed(-1)
    with pytest.raises(ValueError, match="temporal_push: n 1.0 "):
        s.replayed(1.0)
    s.replayed(3)
    assert (s.frames, s.emitted) == (3, 1)
    s.replayed()
    assert (s.frames, s.emitted) == (4, 2)
    s.reset()
    assert (s.frames, s.emitted) == (0, 0)
    assert s.flush() == [] and s.closed                               # a flush after no push: nothing owed, nothing launched
    with pytest.raises(RuntimeError, match=re.escape("temporal_push: a push after flush(): the stream is closed")):
        s.push(good)
    s.reset()
    assert not s.closed and list(s.filter([])) == [] and s.closed
    assert s.sync_frames() == 0                                       # nothing on the device yet: the mirrors stand


# ---- the command lines ----------------------------------------------------------------------------------------------------------------

NEEDED = ["--depth", "d", "--out", "o"]
REG = [*NEEDED, "--calib", "c"]


def test_temporal_parse_args_yields_what_it_yielded():
    """The namespace of the arguments tests/test_temporal_cpu.py passes, attribute by attribute as before add_arguments took the
    filter's flags over; --stream is the one new attribute"""
    a, _, f = K.parse_args(NEEDED)
    assert vars(a) == dict(depth="d", out="o", depth_bits=8, depth_max=None, window=5, causal=False, tolerance=2, tolerance_rel=0.02,
                           min_count=2, min_fill=2, block=256, stats=False, top=255, stream=False)
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (2, 2, 2, RQ, 2, 2)
    a, _, f = K.parse_args([*NEEDED, "--depth-bits", "16", "--depth-max", "10000", "--window", "6", "--causal", "--tolerance", "8",
                            "--tolerance-rel", "0.05", "--min-count", "3", "--min-fill", "0", "--block", "4", "--stats"])
    assert vars(a) == dict(depth="d", out="o", depth_bits=16, depth_max=10000, window=6, causal=True, tolerance=8, tolerance_rel=0.05,
                           min_count=3, min_fill=0, block=4, stats=True, top=10000, stream=False)
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (5, 0, 8, 3277, 3, 0)
    a, _, f = K.parse_args([*NEEDED, "--stream", "--window", "4", "--causal", "--block", "0"])         # --block is not looked at
    assert a.stream and a.block == 0 and (f.back, f.ahead) == (3, 0)


@pytest.mark.parametrize("argv, word", [
    ([*NEEDED, "--stream", "--window", "4"], "--window 4 "),
    ([*NEEDED, "--stream", "--window", "16", "--causal"], "--window 16 "),
    ([*NEEDED, "--stream", "--tolerance", "256"], "--tolerance 256 is above the largest code 255"),
    ([*NEEDED, "--stream", "--min-count", "0"], "--min-count 0 "),
    ([*NEEDED, "--stream", "--min-fill", "16"], "--min-fill 16 "),
    ([*NEEDED, "--stream", "--tolerance-rel", "1.0"], "--tolerance-rel 1.0 "),
    (["--depth", "d", "--out", "./d", "--stream"], "--out is --depth"),
    ([*NEEDED, "--block", "0"], "--block 0 must be in"),
])
def test_stream_command_line_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        K.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


@pytest.mark.parametrize("argv, word", [
    ([*REG, "--temporal-window", "3"], "--temporal-window needs --temporal"),
    ([*REG, "--temporal-causal"], "--temporal-causal needs --temporal"),
    ([*REG, "--temporal-tolerance", "3"], "--temporal-tolerance needs --temporal"),
    ([*REG, "--temporal-tolerance-rel", "0.1"], "--temporal-tolerance-rel needs --temporal"),
    ([*REG, "--temporal-min-count", "3"], "--temporal-min-count needs --temporal"),
    ([*REG, "--temporal-min-fill", "3"], "--temporal-min-fill needs --temporal"),
    ([*REG, "--clean", "--temporal-min-fill", "3"], "--temporal-min-fill needs --temporal"),
    ([*REG, "--temporal", "--temporal-window", "4"], "--temporal-window 4 "),
    ([*REG, "--temporal", "--temporal-window", "16", "--temporal-causal"], "--temporal-window 16 "),
    ([*REG, "--temporal", "--temporal-tolerance", "-1"], "--temporal-tolerance -1 "),
    ([*REG, "--temporal", "--temporal-tolerance", "256"], "--temporal-tolerance 256 is above the largest code 255"),
    ([*REG, "--temporal", "--temporal-tolerance-rel", "nan"], "--temporal-tolerance-rel nan "),
    ([*REG, "--temporal", "--temporal-min-count", "16"], "--temporal-min-count 16 "),
    ([*REG, "--temporal", "--temporal-min-fill", "-1"], "--temporal-min-fill -1 "),
    ([*REG, "--temporal", "--clean-min-region", "3"], "--clean-min-region needs --clean"),
])
def test_register_temporal_refusals(capsys, argv, word):
    with pytest.raises(SystemExit) as e:
        P.parse_args(argv)
    assert e.value.code == 2 and re.search(word, capsys.readouterr().err)


def test_register_temporal_arguments():
    a, _ = P.parse_args(REG)
    assert a.temporal is False and a.temporal_filter is None and a.cleaner is None
    a, _ = P.parse_args([*REG, "--temporal"])
    f = a.temporal_filter
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (2, 2, 2, RQ, 2, 2) and a.cleaner is None
    a, _ = P.parse_args([*REG, "--temporal", "--temporal-window", "6", "--temporal-causal", "--temporal-tolerance", "8",
                         "--temporal-tolerance-rel", "0.05", "--temporal-min-count", "3", "--temporal-min-fill", "0", "--clean",
                         "--clean-tolerance", "4", "--depth-bits", "16", "--depth-max", "10000"])
    f = a.temporal_filter
    assert (f.back, f.ahead, f.tolerance, f.tolerance_rel_q16, f.min_count, f.min_fill) == (5, 0, 8, 3277, 3, 0)
    assert a.cleaner.tolerance == 4
