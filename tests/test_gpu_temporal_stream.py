"""The temporal stream on the MI355X (codon_amd.temporal.TemporalStream, codon_temporal_push) against the numpy
restatement tests/temporal_ref.py of the WHOLE sequence (pinned on the CPU by tests/test_temporal_cpu.py) -- never against the
sequence kernel.  The bar is EQUAL BITS, codes and statistics, no tolerance anywhere: frame t is final once frame t + ahead is in.
Cases (tests/temporal_stream_cases.py): the planes of temporal_ref.PLANES under all seven windows at the lengths 1, 2, ahead,
ahead + 1, 15, 16, 17 and 33 -- every output from the flush, a full ring, a wrapped one, one wrapped twice -- the large plane at
1, 3 and 17; parameters, patterns and formats in turn."""
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
from tests import temporal_stream_cases as S
from tests.test_temporal_stream_cpu import RQ, check_push_refusals, push_caller

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
    return f


def _stream(case):
    T, h, w, *_, top = case
    return K.TemporalStream(_filter(case), (h, w), torch.uint8 if top == 255 else torch.int16, None if top == 255 else top)


def _run(s, src, stats=True):
    """Push every frame of src (T, h, w) and flush -> (codes (T, h, w), counts (T, 4) or None), checking what each step answers"""
    outs = []
    for t in range(src.shape[0]):
        got = s.push(src[t], stats=stats)
        assert (got is None) == (t < s.latency) and s.frames == t + 1 and s.emitted == max(0, t + 1 - s.latency)
        if got is not None:
            outs.append(got)
    rest = s.flush(stats=stats)
    assert len(rest) == min(s.latency, src.shape[0]) and s.emitted == s.frames == src.shape[0] and s.closed
    outs += rest
    if not stats:
        return torch.stack(outs), None
    return torch.stack([o for o, _ in outs]), torch.stack([c for _, c in outs])


@pytest.mark.parametrize("plane", R.PLANES, ids=ids)
def test_equals_the_restatement(plane):
    """Every case of one plane: each emitted frame and its statistics row equal the restatement of the whole sequence; no frame is
    modified; after reset() the same object filters the sequence again without statistics, through filter(), to the same codes"""
    rows = [c for c in S.cases() if c[1:3] == plane]
    assert len(rows) >= 21
    for case in rows:
        want, stats = R.want(case)
        src = _codes_dev(R.sequence(case[0], *plane, case[9], case[10]))
        before = src.clone()
        s = _stream(case)
        got, counts = _run(s, src)
        assert got.shape == want.shape and got.dtype == src.dtype and counts.shape == (case[0], 4) and counts.dtype == torch.int32
        bad = np.argwhere(_bits(got) != want)
        assert bad.size == 0, f"{case}: {len(bad)} codes differ, first at {bad[:3].tolist()}"
        assert np.array_equal(_bits(counts), stats), (case, _bits(counts).tolist(), stats.tolist())
        s.reset()
        again = list(s.filter(src))
        assert len(again) == case[0] and torch.equal(torch.stack(again), got) and torch.equal(src, before)
        assert s.sync_frames() == case[0] and s.emitted == case[0]


def test_reset_and_a_second_sequence_and_uint16():
    """One object, three sequences in a row: what an earlier one left in the ring and the counters is not seen"""
    T, h, w, top = 17, 40, 100, 10000
    A = R.SCENE_TOLERANCE[top]
    s = K.TemporalStream(K.TemporalFilter(tolerance=A), (h, w), torch.int16, top)
    for pattern in ("random", "scene", "single"):
        want, stats = R.temporal(R.sequence(T, h, w, pattern, top), 2, 2, A, RQ, 2, 2)
        got, counts = _run(s, _codes_dev(R.sequence(T, h, w, pattern, top)))
        assert np.array_equal(_bits(got), want) and np.array_equal(_bits(counts), stats), pattern
        s.reset()
    u = K.TemporalStream(K.TemporalFilter(tolerance=A), (h, w), torch.uint16, top)
    src16 = _codes_dev(R.sequence(T, h, w, "single", top)).view(torch.uint16)
    outs = list(u.filter(src16[t] for t in range(T)))
    assert len(outs) == T and all(o.dtype == torch.uint16 for o in outs)
    assert np.array_equal(_bits(torch.stack([o.view(torch.int16) for o in outs])), want)


def test_two_streams_do_not_see_each_other():
    """Two streams of different windows and sequences interleaved on one HIP stream, and two on two HIP streams"""
    T, h, w, top = 17, 9, 29, 65535
    A = R.SCENE_TOLERANCE[top]
    a, b = R.sequence(T, h, w, "random", top), R.sequence(T, h, w, "high", top)
    want_a, stats_a = R.temporal(a, 2, 2, A, RQ, 2, 2)
    want_b, stats_b = R.temporal(b, 7, 0, A, RQ, 2, 2)
    da, db = _codes_dev(a), _codes_dev(b)

    def both(streams):
        sa = K.TemporalStream(K.TemporalFilter(tolerance=A), (h, w), torch.int16)
        sb = K.TemporalStream(K.TemporalFilter(tolerance=A, window=8, causal=True), (h, w), torch.int16)
        oa, ob = [], []
        for t in range(T):
            for s, d, o, stream in ((sa, da, oa, streams[0]), (sb, db, ob, streams[1])):
                with torch.cuda.stream(stream):
                    got = s.push(d[t], stats=True)
                    if got is not None:
                        o.append(got)
        for s, o, stream in ((sa, oa, streams[0]), (sb, ob, streams[1])):
            with torch.cuda.stream(stream):
                o += s.flush(stats=True)
        torch.cuda.synchronize()
        for o, want, stats in ((oa, want_a, stats_a), (ob, want_b, stats_b)):
            assert np.array_equal(_bits(torch.stack([x for x, _ in o])), want)
            assert np.array_equal(_bits(torch.stack([c for _, c in o])), stats)

    one = torch.cuda.current_stream()
    both((one, one))
    torch.cuda.synchronize()
    both((torch.cuda.Stream(), torch.cuda.Stream()))


def test_a_callers_out_buffer():
    """out= is written and returned once a frame is final, and left as it was while the answer is None"""
    T, h, w, top = 5, 5, 7, 255
    c = R.sequence(T, h, w, "all", top)
    want, stats = R.temporal(c, 2, 2, 1, RQ, 2, 2)
    s = K.TemporalStream(K.TemporalFilter(tolerance=1), (h, w), torch.uint8)
    src = _codes_dev(c)
    out = torch.full((h, w), 99, dtype=torch.uint8, device="cuda")
    for t in range(T):
        got = s.push(src[t], out=out)
        if t < 2:
            assert got is None and (out == 99).all()
        else:
            assert got is out and np.array_equal(_bits(out), want[t - 2])
    got, counts = s.flush(stats=True)[1]
    assert np.array_equal(_bits(got), want[4]) and np.array_equal(_bits(counts), stats[4])


@pytest.mark.parametrize("top", [255, 10000])
def test_frames_one_element_into_larger_buffers(top):
    """in and out one element into larger buffers (u8: an odd address; u16: two bytes off every wider alignment) on a plane of whole
    quads: the four-pixel loads and stores must not be taken; the elements before and behind stay as they were"""
    lib = L.load()
    T, h, w = 17, 40, 100
    n = h * w
    A = R.SCENE_TOLERANCE[top]
    c = R.sequence(T, h, w, "random", top)
    want, stats = R.temporal(c, 2, 5, A, RQ, 2, 2)
    dt = torch.uint8 if top == 255 else torch.int16
    fmt = L.FILL_U8 if top == 255 else L.FILL_U16
    dev = _codes_dev(c).reshape(T, n)
    src = torch.full((n + 2,), 77, dtype=dt, device="cuda")
    out = torch.full((n + 2,), 99, dtype=dt, device="cuda")
    ring = torch.empty((16, n), dtype=dt, device="cuda")
    state = torch.zeros(2, dtype=torch.int32, device="cuda")
    counts = torch.empty(4, dtype=torch.int32, device="cuda")
    e = src.element_size()
    stream = ops._stream(torch.device("cuda:0"))
    outs, rows = [], []
    for step in range(T + 5):
        if step < T:
            src[1:n + 1] = dev[step]
        st = lib.codon_temporal_push(h, w, src.data_ptr() + e if step < T else None, fmt, top, 2, 5, A, RQ, 2, 2, ring.data_ptr(),
                                     state.data_ptr(), out.data_ptr() + e, counts.data_ptr(), stream)
        L.check(st, "temporal_push")
        if step >= 5:
            outs.append(out[1:n + 1].clone())
            rows.append(counts.clone())
    torch.cuda.synchronize()
    assert np.array_equal(_bits(torch.stack(outs)).reshape(T, h, w), want) and np.array_equal(_bits(torch.stack(rows)), stats)
    assert out[0] == 99 and out[n + 1] == 99 and src[0] == 77 and src[n + 1] == 77
    assert state.tolist() == [T, 5]


@pytest.mark.parametrize("h, w, window", [(5, 7, (2, 2)), (4, 8, (3, 0))], ids=["5x7-2-2", "4x8-3-0"])
def test_one_captured_push_replays_for_every_later_frame(h, w, window):
    """Frame 0 is pushed eagerly; the push of frame 1 is captured once, on one stream, and replayed for frames 1 .. 16 on changed
    contents of the same input tensor -- the frame index lives on the device; then replayed(15) and an eager flush.  Equal to the
    eager stream and to the restatement"""
    T, top = 17, 65535
    A = R.SCENE_TOLERANCE[top]
    c = R.sequence(T, h, w, "random", top)
    want, stats = R.temporal(c, *window, A, RQ, 2, 2)
    filt = K.TemporalFilter(tolerance=A, back=window[0], ahead=window[1])
    src = _codes_dev(c)
    eager, eager_counts = _run(K.TemporalStream(filt, (h, w), torch.int16), src)
    s = K.TemporalStream(filt, (h, w), torch.int16)
    frame = src[0].clone()
    out = torch.zeros((h, w), dtype=torch.int16, device="cuda")
    first = s.push(frame, stats=True)
    outs = [first] if first is not None else []
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        got, counts = s.push(frame, stats=True, out=out)
    assert got is out and s.frames == 2
    for t in range(1, T):
        frame.copy_(src[t])
        graph.replay()
        if t >= window[1]:
            outs.append((out.clone(), counts.clone()))
    s.replayed(T - 2)
    assert (s.frames, s.emitted) == (T, T - window[1])
    outs += s.flush(stats=True)
    torch.cuda.synchronize()
    assert s.sync_frames() == T and s.emitted == T
    codes, rows = torch.stack([o for o, _ in outs]), torch.stack([r for _, r in outs])
    assert torch.equal(codes, eager) and torch.equal(rows, eager_counts)
    assert np.array_equal(_bits(codes), want) and np.array_equal(_bits(rows), stats)


def test_refusals_leave_everything_untouched():
    lib = L.load()
    h, w = 5, 7
    both = torch.full((4096,), -21555, dtype=torch.int16, device="cuda")      # in and out 4096 bytes apart: a ring laid over one
    src, out = both[:h * w].view(h, w), both[2048:2048 + h * w].view(h, w)  # of them (1120 bytes) does not reach the other
    src.copy_(_codes_dev(R.sequence(3, h, w, "random", 65535))[0])
    ring = torch.full((16, h, w), 4242, dtype=torch.int16, device="cuda")
    state = torch.full((2,), 7, dtype=torch.int32, device="cuda")
    counts = torch.full((4,), -7, dtype=torch.int32, device="cuda")
    keep = src.clone()
    call = push_caller(lib, src.data_ptr(), ring.data_ptr(), state.data_ptr(), out.data_ptr(), counts.data_ptr(),
                       ops._stream(torch.device("cuda:0")))
    check_push_refusals(lib, call, src.data_ptr(), out.data_ptr())
    assert "unaligned" in call(src=src.data_ptr() + 1)[1] and "unaligned" in call(counts=counts.data_ptr() + 2)[1]
    assert "unaligned" in call(state=state.data_ptr() + 2)[1] and "unaligned" in call(ring=ring.data_ptr() + 1)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and (ring == 4242).all() and (state == 7).all() and (counts == -7).all() and torch.equal(src, keep)
    state.zero_()
    assert call(back=0, ahead=0, tol_abs=R.SCENE_TOLERANCE[65535])[0] == 0           # and the good call goes through
    torch.cuda.synchronize()
    assert state.tolist() == [1, 0] and torch.equal(out, src) and torch.equal(ring[0], src) and (ring[1:] == 4242).all()
    assert counts.tolist() == [int((src != 0).sum()), 0, 0, 0]


def test_flush_after_no_push_and_a_push_after_a_flush():
    s = K.TemporalStream(K.TemporalFilter(), (5, 7), torch.uint8)
    frame = torch.zeros((5, 7), dtype=torch.uint8, device="cuda")
    assert s.flush() == [] and s.closed
    with pytest.raises(RuntimeError, match="temporal_push: a push after flush"):
        s.push(frame)
    s.reset()
    assert s.push(frame) is None and s.push(frame) is None and len(s.flush()) == 2
    with pytest.raises(RuntimeError, match="temporal_push: a push after flush"):
        s.push(frame)
    with pytest.raises(ValueError, match="temporal_push: a frame of shape"):
        K.TemporalStream(K.TemporalFilter(), (5, 7), torch.uint8).push(frame[:4])
    with pytest.raises(RuntimeError, match="temporal_push: out on cpu, the stream on cuda:0"):
        K.TemporalStream(K.TemporalFilter(), (5, 7), torch.uint8).push(frame, out=torch.zeros((5, 7), dtype=torch.uint8))


@pytest.mark.parametrize("top", [255, 65535, 10000])
def test_filter_equals_the_sequence_call(top):
    """TemporalStream.filter on a sequence equals TemporalFilter.__call__ on it and the restatement: the scene on its three grids"""
    c = R.scene(top)[0]
    A = R.SCENE_TOLERANCE[top]
    f = K.TemporalFilter(tolerance=A)
    src, dm = _codes_dev(c), None if top == 255 else top
    s = K.TemporalStream(f, c.shape[1:], src.dtype, dm)
    got = torch.stack(list(s.filter(src)))
    want, stats = R.temporal(c, 2, 2, A, RQ, 2, 2)
    assert torch.equal(got, f(src, dm)) and np.array_equal(_bits(got), want)
    s.reset()
    rows = torch.stack([r for _, r in s.filter(src, stats=True)])
    assert np.array_equal(_bits(rows), stats) and stats[:, 1].sum() == 60 and stats[:, 2].sum() == 660


def test_a_sequence_the_call_refuses_for_length():
    """4097 frames: TemporalFilter.__call__ refuses them, the stream runs them.  The expectation: the restatement of frames
    0 .. 4095 for the outputs whose windows lie inside them and of frames 1 .. 4096 for the others -- the definition reads nothing
    beyond a window (tests/test_temporal_cpu.py proves it of blocks)"""
    T, h, w, top = 4097, 1, 5, 10000
    g = np.random.default_rng(24)
    c = np.where(g.random((T, h, w)) < 0.3, 0, 5000 + g.integers(-2, 3, size=(T, h, w))).astype(np.uint16)
    f = K.TemporalFilter(tolerance=2)
    src = _codes_dev(c)
    with pytest.raises(ValueError, match="temporal_depth: a sequence of 4097 frames"):
        f(src, top)
    head, hstats = R.temporal(c[:4096], 2, 2, 2, RQ, 2, 2)
    tail, tstats = R.temporal(c[1:], 2, 2, 2, RQ, 2, 2)
    want = np.concatenate([head[:4000], tail[3999:]])
    stats = np.concatenate([hstats[:4000], tstats[3999:]])
    got, counts = _run(K.TemporalStream(f, (h, w), torch.int16, top), src)
    assert np.array_equal(_bits(got), want) and np.array_equal(_bits(counts), stats)


# ---- the command lines -----------------------------------------------------------------------------------------------------------------

def _files(tmp_path, bits, top, T=9):
    shape = G.SHAPES[5]                                               # 70 x 130 onto 35 x 65 at scale 4 of 140 x 260
    sensor = str(tmp_path / "sensor")
    os.makedirs(sensor)
    write = io.write_gray if bits == 8 else io.write_depth16
    c = R.sequence(T, *shape[1:3], "scene", top)
    names = [f"{i:02d}.png" for i in range(T)]
    for name, frame in zip(names, c):
        write(os.path.join(sensor, name), frame)
    return shape, sensor, names, c, ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []


def _same_files(a, b, names):
    assert sorted(os.listdir(a)) == sorted(os.listdir(b)) == names
    for name in names:
        assert open(os.path.join(a, name), "rb").read() == open(os.path.join(b, name), "rb").read(), name


@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_stream_writes_the_default_modes_bytes_and_lines(tmp_path, capsys, bits, top):
    """temporal.main --stream on nine files: the files and the emitted lines, --stats included, are byte for byte those of the
    default mode, under a centred and a causal window; a file of another shape is refused by name"""
    _, sensor, names, c, fmt = _files(tmp_path, bits, top)
    A = R.SCENE_TOLERANCE[top]
    for k, window in enumerate((["--window", "5"], ["--window", "4", "--causal"], ["--window", "5", "--stats"])):
        whole, live = str(tmp_path / f"whole{k}"), str(tmp_path / f"live{k}")
        capsys.readouterr()
        assert K.main(["--depth", sensor, "--out", whole, "--tolerance", str(A), *window, *fmt]) == 0
        lines = capsys.readouterr().out
        assert K.main(["--depth", sensor, "--out", live, "--tolerance", str(A), "--stream", *window, *fmt]) == 0
        assert capsys.readouterr().out == lines and len(lines.splitlines()) == len(names)
        _same_files(whole, live, names)
    want, stats = R.temporal(c, 2, 2, A, RQ, 2, 2)
    for i, name in enumerate(names):
        assert np.array_equal(io.read_depth_plane(os.path.join(live, name), bits, top), want[i]), i
        v, r, f, ch = (int(x) for x in stats[i])
        assert lines.splitlines()[i] == f"{name} valid={v} rejected={r} filled={f} changed={ch}"
    (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(sensor, "zz.png"), c[0][:-1])
    with pytest.raises(SystemExit) as e:
        K.main(["--depth", sensor, "--out", str(tmp_path / "odd"), "--stream", *fmt])
    assert e.value.code == 2 and "zz.png is 69x130, 00.png is 70x130" in capsys.readouterr().err


@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_register_temporal_writes_the_chains_bytes(tmp_path, capsys, bits, top):
    """register.main --temporal --clean --stats writes the bytes of temporal.main, clean.main and register.main run in a row, and
    prints their statistics on one line; without --clean, those of temporal.main and register.main"""
    shape, sensor, names, c, fmt = _files(tmp_path, bits, top)
    A = R.SCENE_TOLERANCE[top]
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(G.calibration(shape, "mixed")))
    filtered, cleaned, chain, chain2, one, two = (str(tmp_path / n) for n in ("filtered", "cleaned", "chain", "chain2", "one", "two"))
    reg = ["--calib", str(rig), "--scale", "4", "--depth-unit", repr(G.unit_of(top)), *fmt]

    def lines_of(run, argv):
        capsys.readouterr()
        assert run(argv) == 0
        return capsys.readouterr().out.strip().splitlines()

    t_lines = lines_of(K.main, ["--depth", sensor, "--out", filtered, "--window", "3", "--tolerance", str(A), "--stats", *fmt])
    c_lines = lines_of(clean.main, ["--depth", filtered, "--out", cleaned, "--tolerance", str(A), "--stats", *fmt])
    r_lines = lines_of(P.main, ["--depth", cleaned, "--out", chain, "--stats", *reg])
    got = lines_of(P.main, ["--depth", sensor, "--out", one, "--stats", "--temporal", "--temporal-window", "3", "--temporal-tolerance",
                            str(A), "--clean", "--clean-tolerance", str(A), *reg])
    _same_files(chain, one, names)
    tail = lambda line, name: line[len(name) + 1:]                   # noqa: E731
    assert got == [f"{r} temporal: {tail(t, n)} cleaned: {tail(k, n)}" for n, t, k, r in zip(names, t_lines, c_lines, r_lines)]
    assert " temporal: valid=" in got[0] and " cleaned: valid=" in got[0] and got[0].startswith("00.png valid=")
    r_lines = lines_of(P.main, ["--depth", filtered, "--out", chain2, *reg])
    got = lines_of(P.main, ["--depth", sensor, "--out", two, "--temporal", "--temporal-window", "3", "--temporal-tolerance", str(A), *reg])
    _same_files(chain2, two, names)
    assert got == r_lines == names
