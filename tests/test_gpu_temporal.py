"""The temporal filter of a fixed camera's depth sequence on the MI355X against the numpy restatement
tests/temporal_ref.py (pinned on the CPU by tests/test_temporal_cpu.py).  The bar is EQUAL BITS, codes and statistics, no tolerance
anywhere.
Planes (temporal_ref.PLANES), the smallest at which each part can go wrong: one pixel; a single row of 37; 5 x 7; 17 x 17; 40 x 100
(four pixel groups, whole quads: the four-pixel loads and stores); 9 x 29 (a width one more than a multiple of a thread's four
pixels, a partial last quad); 4 x 8 (whole quads under the long sequences).  Lengths: 1, 2, 3, 15, 16, 17 and, from the library's own
chunk rule, one frame less than a time chunk, a chunk, one more, and two chunks and one -- the long ones on the small planes.
Windows, parameters, patterns and formats in turn (temporal_ref.cases)."""
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import clean, io, ops
from codon_amd import register as P
from codon_amd import temporal as K
from tests import register_ref as G
from tests import temporal_ref as R
from tests.test_temporal_cpu import RQ, temporal_caller, temporal_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _filter(case):
    T, h, w, Bk, Ah, M, F, A, Rq, pattern, top = case
    f = K.TemporalFilter(tolerance=A, tolerance_rel=Rq / 65536.0, min_count=M, min_fill=F, back=Bk, ahead=Ah)
    assert f.tolerance_rel_q16 == Rq
    return f, _codes_dev(R.sequence(T, h, w, pattern, top)), None if top == 255 else top


@pytest.mark.parametrize("plane", R.PLANES, ids=ids)
def test_equals_the_restatement(plane):
    """temporal_ref.cases of one plane (the scene's three with its own): codes and statistics; no argument is modified; a call
    without statistics gives the same codes"""
    rows = [c for c in R.cases() if c[1:3] == plane]
    assert len(rows) >= 28
    for case in rows:
        want, stats = R.want(case)
        f, src, dm = _filter(case)
        before = src.clone()
        got, counts = f(src, dm, stats=True)
        assert got.shape == want.shape and got.dtype == src.dtype and got.is_contiguous()
        assert counts.shape == (case[0], 4) and counts.dtype == torch.int32
        bad = np.argwhere(_bits(got) != want)
        assert bad.size == 0, f"{case}: {len(bad)} codes differ, first at {bad[:3].tolist()}"
        assert np.array_equal(_bits(counts), stats), (case, _bits(counts).tolist(), stats.tolist())
        assert torch.equal(f(src, dm), got) and torch.equal(src, before)


def test_the_lengths_stand_on_both_sides_of_the_librarys_chunk():
    """The case set's lengths come from tests/temporal_ref.chunk_frames; the library's own rule puts them where they are meant to be:
    one chunk at L - 1 and L, two at L + 1, three at 2 L + 1, and a window that reads across the seam"""
    q = L.load().codon_temporal_chunk_frames
    for plane in R.PLANES[:4]:
        for Bk, Ah in R.WINDOWS:
            ln = q(R.MAX_FRAMES, *plane, Bk, Ah)
            assert ln == R.chunk_frames(R.MAX_FRAMES, *plane, Bk, Ah) and {ln - 1, ln, ln + 1, 2 * ln + 1} <= set(R.lengths(plane, (Bk, Ah)))
            chunks = lambda T: -(-T // q(T, *plane, Bk, Ah))         # noqa: E731
            assert [chunks(T) for T in (ln - 1, ln, ln + 1, 2 * ln + 1)] == [1, 1, 2, 3]
    assert sum(1 for T, h, w, Bk, Ah, *_ in R.cases() if Bk + Ah > 0 and q(T, h, w, Bk, Ah) < T) > 50


def test_a_second_call_plane_forms_and_two_streams():
    """A second call on the same stream with another sequence equals its own restatement, whatever the first left behind; an
    (h, w) plane is a sequence of one frame; uint16 tensors; two streams"""
    T, h, w, top = 17, 40, 100, 10000
    f = K.TemporalFilter(tolerance=R.SCENE_TOLERANCE[top])
    ref = lambda pattern: R.temporal(R.sequence(T, h, w, pattern, top), 2, 2, R.SCENE_TOLERANCE[top], RQ, 2, 2)     # noqa: E731
    first = f(_codes_dev(R.sequence(T, h, w, "random", top)), top)
    for pattern in ("all", "scene", "none", "single", "random"):
        want, stats = ref(pattern)
        got, counts = f(_codes_dev(R.sequence(T, h, w, pattern, top)), top, stats=True)
        assert np.array_equal(_bits(got), want) and np.array_equal(_bits(counts), stats), pattern
    assert torch.equal(got, first)
    dev = _codes_dev(R.sequence(T, h, w, "random", top))
    one, c1 = f(dev[0], top, stats=True)
    w1, s1 = R.temporal(R.sequence(T, h, w, "random", top)[:1], 2, 2, R.SCENE_TOLERANCE[top], RQ, 2, 2)
    assert one.shape == (h, w) and one.dtype == torch.int16 and np.array_equal(_bits(one), w1[0]) and np.array_equal(_bits(c1), s1)
    u16 = f(dev.view(torch.uint16), top)
    assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want)
    torch.cuda.synchronize()
    outs = []
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            outs.append(f(dev, top, stats=True))
    torch.cuda.synchronize()
    for out, counts in outs:
        assert np.array_equal(_bits(out), want) and np.array_equal(_bits(counts), stats)
    with pytest.raises(RuntimeError, match="temporal_depth expects"):
        f(dev.float(), top)
    with pytest.raises(ValueError, match="temporal_depth: depth_max 10000 with 8-bit codes"):
        f(dev.to(torch.uint8), top)
    with pytest.raises(ValueError, match="temporal_depth: tolerance 8 above the largest code 5"):
        f(dev, 5)


def test_capture_and_replay():
    """One call inside a capture (a single branch: two launches in a row on the capture's stream) and one replay equal the eager
    call; the replay runs on other contents of the same input tensor"""
    T, h, w, top = 16, 40, 100, 65535
    f = K.TemporalFilter(tolerance=R.SCENE_TOLERANCE[top])
    a, b = _codes_dev(R.sequence(T, h, w, "random", top)), _codes_dev(R.scene(top)[0])
    eager = f(b, stats=True)
    src = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, counts = f(src, stats=True)
    src.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(counts, eager[1])
    want, stats = R.temporal(R.scene(top)[0], 2, 2, R.SCENE_TOLERANCE[top], RQ, 2, 2)
    assert np.array_equal(_bits(out), want) and np.array_equal(_bits(counts), stats)
    assert stats[:, 1].sum() == 60 and stats[:, 2].sum() == 660


@pytest.mark.parametrize("top", [255, 10000])
def test_sequences_one_element_into_larger_buffers(top):
    """src and out one element into larger buffers (u8: an odd address; u16: two bytes off every wider alignment) on a plane of
    whole quads: the four-pixel loads and stores must not be taken; the elements before and behind stay as they were"""
    lib = L.load()
    T, h, w = 17, 40, 100
    n = T * h * w
    A = R.SCENE_TOLERANCE[top]
    c = R.sequence(T, h, w, "random", top)
    want, stats = R.temporal(c, 2, 5, A, RQ, 2, 2)
    dt = torch.uint8 if top == 255 else torch.int16
    src = torch.full((n + 2,), 77, dtype=dt, device="cuda")
    src[1:n + 1] = _codes_dev(c).reshape(-1)
    out = torch.full((n + 2,), 99, dtype=dt, device="cuda")
    counts = torch.empty((T, 4), dtype=torch.int32, device="cuda")
    e = src.element_size()
    st = lib.codon_temporal_depth(T, h, w, src.data_ptr() + e, L.FILL_U8 if top == 255 else L.FILL_U16, top, 2, 5, A, RQ, 2, 2,
                                  out.data_ptr() + e, counts.data_ptr(), ops._stream(torch.device("cuda:0")))
    L.check(st, "temporal_depth")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[1:n + 1]).reshape(T, h, w), want) and np.array_equal(_bits(counts), stats)
    assert out[0] == 99 and out[n + 1] == 99 and src[0] == 77 and src[n + 1] == 77


def test_refusals_leave_out_untouched():
    lib = L.load()
    src = _codes_dev(R.sequence(3, 5, 7, "random", 65535))
    out = torch.full((4, 5, 7), -21555, dtype=torch.int16, device="cuda")
    counts = torch.full((4, 4), -7, dtype=torch.int32, device="cuda")
    keep = src.clone()
    call = temporal_caller(lib, src.data_ptr(), out.data_ptr(), counts.data_ptr(), ops._stream(torch.device("cuda:0")))
    temporal_refusals(lib, call)
    assert "unaligned" in call(src=src.data_ptr() + 1)[1] and "unaligned" in call(counts=counts.data_ptr() + 2)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and (counts == -7).all() and torch.equal(src, keep)
    assert call(tol_abs=R.SCENE_TOLERANCE[65535])[0] == 0              # and the good call goes through
    want, st = R.temporal(R.sequence(3, 5, 7, "random", 65535), 2, 2, R.SCENE_TOLERANCE[65535], RQ, 2, 2)
    assert np.array_equal(_bits(out[:3]), want) and (out[3] == -21555).all()
    assert np.array_equal(_bits(counts[:3]), st) and (counts[3] == -7).all()


# ---- the command line, and clean and register on what it wrote ---------------------------------------------------------------------------

@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_writes_what_clean_and_register_read(tmp_path, capsys, bits, top):
    """temporal.main on nine files writes PNGs equal to the restatement of the whole sequence and prints the statistics; --block 4
    writes the bytes of --block 256; clean.main reads the result and register.main reads clean's"""
    shape = G.SHAPES[5]                                               # 70 x 130 onto 35 x 65 at scale 4 of 140 x 260
    hs, ws = shape[1:3]
    T, A = 9, R.SCENE_TOLERANCE[top]
    sensor, whole, parts, cleaned, lr = (str(tmp_path / n) for n in ("sensor", "whole", "parts", "cleaned", "lr"))
    os.makedirs(sensor)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(G.calibration(shape, "mixed")))
    write = io.write_gray if bits == 8 else io.write_depth16
    c = R.sequence(T, hs, ws, "scene", top)
    names = [f"{i:02d}.png" for i in range(T)]
    for name, frame in zip(names, c):
        write(os.path.join(sensor, name), frame)
    want, stats = R.temporal(c, 2, 2, A, RQ, 2, 2)
    fmt = ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []
    capsys.readouterr()
    assert K.main(["--depth", sensor, "--out", whole, "--tolerance", str(A), "--stats", *fmt]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert K.main(["--depth", sensor, "--out", parts, "--tolerance", str(A), "--stats", "--block", "4", *fmt]) == 0
    assert capsys.readouterr().out.strip().splitlines() == lines and len(lines) == T
    for i, name in enumerate(names):
        got = io.read_depth_plane(os.path.join(whole, name), bits, top)
        assert got.dtype == want.dtype and np.array_equal(got, want[i]), i
        assert open(os.path.join(parts, name), "rb").read() == open(os.path.join(whole, name), "rb").read(), i
        v, r, f, ch = (int(x) for x in stats[i])
        assert lines[i] == f"{name} valid={v} rejected={r} filled={f} changed={ch}"
    assert stats[:, 1].sum() > 0 and stats[:, 2].sum() > 0            # the scene: rejection and filling at work
    assert K.main(["--depth", sensor, "--out", str(tmp_path / "quiet"), "--window", "3", "--causal", *fmt]) == 0
    assert capsys.readouterr().out.strip().splitlines() == names
    write(os.path.join(sensor, "zz.png"), c[0][:-1])
    with pytest.raises(SystemExit) as e:
        K.main(["--depth", sensor, "--out", str(tmp_path / "odd"), *fmt])
    assert e.value.code == 2 and "zz.png is 69x130, 00.png is 70x130" in capsys.readouterr().err
    assert clean.main(["--depth", whole, "--out", cleaned, "--tolerance", str(A), *fmt]) == 0
    reg = ["--calib", str(rig), "--scale", "4", "--depth-unit", repr(G.unit_of(top)), *fmt]
    assert P.main(["--depth", cleaned, "--out", lr, *reg]) == 0
    assert sorted(os.listdir(lr)) == names
    assert io.read_depth_plane(os.path.join(lr, names[0]), bits, top).shape == (35, 65)
