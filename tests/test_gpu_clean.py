"""The outlier rejection of sensor depth maps on the MI355X against the numpy restatement tests/clean_ref.py (pinned
on the CPU by tests/test_clean_cpu.py).  The bar is EQUAL BITS, codes and statistics, no tolerance anywhere: counts and component
sizes do not depend on the order of the union-find's atomics.
Shapes (clean_ref.SHAPES), the smallest at which each part can go wrong: one pixel; a single row; odd sizes below a tile; exactly
one 16 x 16 tile; one tile plus one pixel each way (a component crosses a tile corner); a batch of three odd planes; the scene's
size as a batch of two; 93 x 116, many tiles with rows that are not 16-byte aligned and three runs of the apply launch.
Every shape under every pattern and every parameter form (clean_ref.cases), the formats in turn."""
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import clean as K
from codon_amd import infer, io, ops
from codon_amd import register as P
from tests import clean_ref as R
from tests import register_ref as G
from tests.test_clean_cpu import clean_caller, clean_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _cleaner(shape, form, top, pattern=None):
    A, Rq, Kk, N = R.params(shape, form, top, pattern)
    c = K.Cleaner(A, Rq / 65536.0, Kk, N)
    assert c.tolerance_rel_q16 == Rq
    return c


@pytest.mark.parametrize("shape", R.SHAPES, ids=ids)
def test_equals_the_restatement(shape):
    """clean_ref.cases: every pattern under every parameter form, the formats in turn -- codes and statistics; no argument is
    modified; a call without statistics gives the same codes"""
    for name, top, pattern, form in R.cases(shape):
        want, stats = R.want(shape, pattern, top, form)
        src = _codes_dev(R.plane(shape, pattern, top))
        before = src.clone()
        clean = _cleaner(shape, form, top, pattern)
        dm = None if top == 255 else top
        got, counts = clean(src, dm, stats=True)
        assert got.shape == want.shape and got.dtype == src.dtype and got.is_contiguous()
        assert counts.shape == (shape[0], 4) and counts.dtype == torch.int32
        bad = np.argwhere(_bits(got) != want)
        assert bad.size == 0, f"{shape} {name} {pattern} {form}: {len(bad)} codes differ, first at {bad[:3].tolist()}"
        assert np.array_equal(_bits(counts), stats), (shape, name, pattern, form, _bits(counts).tolist(), stats.tolist())
        assert torch.equal(clean(src, dm), got) and torch.equal(src, before)


def test_what_the_case_set_covers():
    """From the restatement: both rules remove something in one call; a component spans more than one tile; a blob of exactly N
    pixels survives and one of N - 1 does not; more than 1000 regions are removed in one image; codes of 32768 and above occur"""
    both, most = 0, 0
    for shape in R.SHAPES:
        for name, top, pattern, form in R.cases(shape):
            _, stats = R.want(shape, pattern, top, form)
            both += int(((stats[:, 1] > 0) & (stats[:, 2] > 0)).any())
            most = max(most, int(stats[:, 3].max()))
    assert both > 0 and most > 1000
    shape = R.SHAPES[4]                                               # 17 x 17: the serpentine is one component through all four tiles
    A, Rq, _, _ = R.params(shape, "default", 10000)
    lab = R.components(R.plane(shape, "serpentine", 10000)[0].astype(np.int64), A, Rq)
    i, j = np.nonzero(lab == 0)
    assert len({(y // R.TILE, x // R.TILE) for y, x in zip(i, j)}) == 4
    shape, top = R.SHAPES[6], 10000                                   # 40 x 100: blobs of 15, 16 and 17 pixels across tile corners
    c, (out, _) = R.plane(shape, "threshold", top), R.want(shape, "threshold", top, "default")
    assert R.THRESHOLD_N == R.params(shape, "default", top)[3] == 16
    blob = lambda a, b: (slice(0, 1), slice(8 * a + 4, 8 * a + 9), slice(8 * b + 5, 8 * b + 9))           # noqa: E731
    assert (c[blob(1, 2)] != 0).sum() == 15 and not out[blob(1, 2)].any()          # rows 13 .. 16, columns 21 .. 24
    assert (c[blob(1, 3)] != 0).sum() == 16 and (out[blob(1, 3)] == c[blob(1, 3)]).all()
    assert (c[blob(1, 1)] != 0).sum() == 17 and (out[blob(1, 1)] == c[blob(1, 1)]).all()                   # across (16, 16)
    assert R.plane(R.SHAPES[7], "high", 65535).max() == 65535 and (R.plane(R.SHAPES[7], "high", 65535) >= 32768).sum() > 5000


def test_a_second_call_plane_forms_and_two_streams():
    """The workspace is initialised by every call: a second call on the same stream with another plane equals its own restatement,
    whatever the first left behind.  (h, w) planes, uint16 tensors, two streams with a workspace each."""
    shape, top = R.SHAPES[7], 10000
    clean = _cleaner(shape, "default", top)
    first = clean(_codes_dev(R.plane(shape, "checker", top)), top)
    for pattern in ("random", "all", "scene", "none", "checker"):
        want, stats = R.want(shape, pattern, top, "default")
        got, counts = clean(_codes_dev(R.plane(shape, pattern, top)), top, stats=True)
        assert np.array_equal(_bits(got), want) and np.array_equal(_bits(counts), stats), pattern
    assert torch.equal(got, first)
    want, stats = R.want(shape, "random", top, "default")
    dev = _codes_dev(R.plane(shape, "random", top))
    one, c1 = clean(dev[0], top, stats=True)
    assert one.shape == shape[1:] and one.dtype == torch.int16 and np.array_equal(_bits(one), want[0]) and c1.shape == (1, 4)
    u16 = clean(dev.view(torch.uint16), top)
    assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want)
    torch.cuda.synchronize()
    outs = []
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            outs.append(clean(dev, top, stats=True))
    torch.cuda.synchronize()
    for out, counts in outs:
        assert np.array_equal(_bits(out), want) and np.array_equal(_bits(counts), stats)
    with pytest.raises(RuntimeError, match="clean_depth expects"):
        clean(dev.float(), top)
    with pytest.raises(ValueError, match="clean_depth: depth_max 10000 with 8-bit codes"):
        clean(dev.to(torch.uint8), top)
    with pytest.raises(ValueError, match="clean_depth: tolerance 8 above the largest code 5"):
        clean(dev, 5)


def test_capture_and_replay():
    """One call inside a capture (a single branch: four launches in a row on the capture's stream) and one replay equal the eager
    call; the replay runs on other contents of the same input tensor"""
    shape, top = R.SHAPES[6], 65535
    clean = _cleaner(shape, "default", top)
    a, b = _codes_dev(R.plane(shape, "random", top)), _codes_dev(R.plane(shape, "scene", top))
    eager = clean(b, stats=True)
    src = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, counts = clean(src, stats=True)
    src.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(counts, eager[1])
    want, stats = R.want(shape, "scene", top, "default")
    assert np.array_equal(_bits(out), want) and np.array_equal(_bits(counts), stats)
    assert stats[0].tolist() == [R.SCENE_VALID, R.SCENE_FLYING, R.SCENE_SPECKLE, R.SCENE_REGIONS]


@pytest.mark.parametrize("top", [255, 10000])
def test_planes_one_element_into_larger_buffers(top):
    """src and out one element into larger buffers (u8: an odd address; u16: two bytes off every wider alignment): the elements
    before and behind the planes stay as they were"""
    lib = L.load()
    shape = R.SHAPES[5]
    B, h, w = shape
    n = B * h * w
    c = R.plane(shape, "random", top)
    want, stats = R.want(shape, "random", top, "default")
    dt = torch.uint8 if top == 255 else torch.int16
    src = torch.full((n + 2,), 77, dtype=dt, device="cuda")
    src[1:n + 1] = _codes_dev(c).reshape(-1)
    out = torch.full((n + 2,), 99, dtype=dt, device="cuda")
    counts = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.codon_clean_workspace_bytes(B, h, w), dtype=torch.uint8, device="cuda")
    A, Rq, Kk, N = R.params(shape, "default", top)
    e = src.element_size()
    st = lib.codon_clean_depth(B, h, w, src.data_ptr() + e, L.FILL_U8 if top == 255 else L.FILL_U16, top, A, Rq, Kk, N,
                               out.data_ptr() + e, counts.data_ptr(), ws.data_ptr(), ws.numel(), ops._stream(torch.device("cuda:0")))
    L.check(st, "clean_depth")
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[1:n + 1]).reshape(shape), want) and np.array_equal(_bits(counts), stats)
    assert out[0] == 99 and out[n + 1] == 99 and src[0] == 77 and src[n + 1] == 77


def test_refusals_leave_out_untouched():
    lib = L.load()
    shape = R.SHAPES[2]
    src = _codes_dev(R.plane(shape, "random", 65535))
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 5, 7), -21555, dtype=torch.int16, device="cuda")
    counts = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    keep = src.clone()
    call = clean_caller(lib, src.data_ptr(), out.data_ptr(), ws.data_ptr(), counts.data_ptr(), ops._stream(torch.device("cuda:0")))
    clean_refusals(lib, call)
    assert "unaligned" in call(src=src.data_ptr() + 1)[1] and "unaligned" in call(ws=ws.data_ptr() + 8)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and (counts == -7).all() and torch.equal(src, keep)
    assert call(tol_abs=R.SCENE_TOLERANCE[65535])[0] == 0              # and the good call goes through
    want, st = R.want(shape, "random", 65535, "default")
    assert np.array_equal(_bits(out[0]), want[0]) and (out[1] == -21555).all()
    assert np.array_equal(_bits(counts[0]), st[0]) and (counts[1] == -7).all()


# ---- the command lines, and register and infer on what they wrote -------------------------------------------------------------------------

@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_writes_what_register_and_infer_read(tmp_path, capsys, bits, top):
    """clean.main on three files writes PNGs equal to the restatement and prints the statistics; register.main reads them, and
    register.main --clean on the sensor's own files writes the same bytes as the two commands one after the other; infer
    --lr-depth --baseline jbu --fill-holes --fill-guided then runs on the result with the colour images"""
    shape = G.SHAPES[5]                                               # 70 x 130 onto 35 x 65 at scale 4 of 140 x 260
    hs, ws = shape[1:3]
    m = G.calibration(shape, "mixed")
    sensor, cleaned, color, lr, lr2 = (str(tmp_path / n) for n in ("sensor", "cleaned", "color", "lr", "lr2"))
    os.makedirs(sensor), os.makedirs(color)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(m))
    write = io.write_gray if bits == 8 else io.write_depth16
    A, T, Q = G.tables(shape, "mixed", top)
    g = np.random.default_rng(5)
    tol = R.SCENE_TOLERANCE[top]
    wants = []
    for i, pattern in enumerate(("scene", "random", "threshold")):
        c = R.plane((1, hs, ws), pattern, top, seed=2 + i)[0]
        write(os.path.join(sensor, f"{i:02d}.png"), c)
        io.write_gray(os.path.join(color, f"{i:02d}.png"), g.integers(0, 256, size=(140, 260), dtype=np.uint8))
        k, stats = R.clean_plane(c, tol, R.rel_q16(0.02), 3, 16)
        wants.append((k, stats, *G.register_plane(k, A, T, Q, 35, 65, top)))
    fmt = ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []
    capsys.readouterr()
    assert K.main(["--depth", sensor, "--out", cleaned, "--tolerance", str(tol), "--stats", *fmt]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3
    for i, (k, stats, _, _) in enumerate(wants):
        got = io.read_depth_plane(os.path.join(cleaned, f"{i:02d}.png"), bits, top)
        assert got.dtype == k.dtype and np.array_equal(got, k), i
        v, f, s, r = (int(x) for x in stats)
        assert lines[i] == f"{i:02d}.png valid={v} flying={f} speckle={s} regions={r}"
    assert wants[0][1][1] > 0 and wants[0][1][2] > 0                  # the scene: both rules at work
    assert K.main(["--depth", sensor, "--out", str(tmp_path / "quiet"), "--tolerance", str(tol), *fmt]) == 0
    assert capsys.readouterr().out.strip().splitlines() == ["00.png", "01.png", "02.png"]
    reg = ["--calib", str(rig), "--scale", "4", "--depth-unit", repr(G.unit_of(top)), *fmt]
    assert P.main(["--depth", cleaned, "--out", lr, *reg, "--stats"]) == 0
    plain = capsys.readouterr().out.strip().splitlines()
    assert P.main(["--depth", sensor, "--out", lr2, *reg, "--stats", "--clean", "--clean-tolerance", str(tol)]) == 0
    fused = capsys.readouterr().out.strip().splitlines()
    for i, (k, stats, want, rstats) in enumerate(wants):
        a, b = (io.read_depth_plane(os.path.join(d, f"{i:02d}.png"), bits, top) for d in (lr, lr2))
        assert np.array_equal(a, want) and a.tobytes() == b.tobytes(), i
        v, o, d, f = (int(x) for x in rstats)
        assert plain[i] == f"{i:02d}.png valid={v} outside={o} dropped={d} filled={f}"
        assert fused[i] == plain[i] + " cleaned: " + lines[i].split(" ", 1)[1]
    sr = str(tmp_path / "sr")
    rc = infer.main(["--scale", "4", "--lr-depth", lr, "--input-color", color, "--out", sr, "--baseline", "jbu", "--fill-holes",
                     "--fill-guided", *fmt])
    assert rc == 0
    up = io.read_depth_plane(os.path.join(sr, "00.png"), bits, top)
    assert up.shape == (140, 260) and (up != 0).all()
