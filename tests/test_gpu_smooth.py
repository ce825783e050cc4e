"""The spatial smoothing of sensor depth maps on the MI355X against the numpy restatement tests/smooth_ref.py (pinned
on the CPU by tests/test_smooth_cpu.py).  The bar is EQUAL BITS, codes and statistics, no tolerance anywhere.
Planes (smooth_ref.PLANES), with T = 32 the tile's side: one pixel; 1 x 7; 9 x 1; 3 x 3 (smaller than every halo); T x T;
(T - 1) x (T + 1); (T + 1) x (2 T + 1); (2 T + 3) x 67, a width that is no multiple of 16 bytes in either format.  Every plane under
every radius of 1, 2, 4 and every pass count with the pair rule on and off -- calls of one fused launch and calls of several, asked
through the library's own plan query --, sigma, the tolerances, the formats, the patterns and the batch in turn (smooth_ref.cases,
which tools/host_check.py smooth shares)."""
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import clean, io, ops
from codon_amd import register as P
from codon_amd import smooth as K
from tests import register_ref as G
from tests import smooth_ref as R
from tests.test_smooth_cpu import RQ, smooth_caller, smooth_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


def _smoother(case):
    B, h, w, radius, passes, sigma, pairs, A, Rq, pattern, top = case
    f = K.Smoother(radius, passes, sigma, A, Rq / 65536.0, pairs)
    assert f.tolerance_rel_q16 == Rq
    return f, _codes_dev(R.codes_of(case)), None if top == 255 else top


@pytest.mark.parametrize("plane", R.PLANES, ids=ids)
def test_equals_the_restatement(plane):
    """smooth_ref.cases of one plane: codes and statistics; the argument is not modified; a call without statistics and a second
    call give the same bytes"""
    rows = [c for c in R.cases() if c[1:3] == plane]
    assert len(rows) == 18
    for case in rows:
        want, stats = R.want(case)
        f, src, dm = _smoother(case)
        before = src.clone()
        got, counts = f(src, dm, stats=True)
        assert got.shape == want.shape and got.dtype == src.dtype and got.is_contiguous()
        assert counts.shape == (case[0], 4) and counts.dtype == torch.int32
        bad = np.argwhere(_bits(got) != want)
        assert bad.size == 0, f"{case}: {len(bad)} codes differ, first at {bad[:3].tolist()}"
        assert np.array_equal(_bits(counts), stats), (case, _bits(counts).tolist(), stats.tolist())
        again, counts2 = f(src, dm, stats=True)
        assert torch.equal(f(src, dm), got) and torch.equal(again, got) and torch.equal(counts2, counts) and torch.equal(src, before)


def test_the_cases_stand_on_both_sides_of_the_librarys_fusion_bound():
    """The library's plan, asked without a launch, is the restatement's; among the cases are calls whose passes all run in one
    launch (the fused side of the bound) and calls of two and of three launches, which go through the workspace (the other side)"""
    for radius in (1, 2, 3, 4):
        for passes in (1, 2, 3):
            p = K.plan(radius, passes)
            assert (p["tile"], p["fuse_bound"], p["launches"]) == (R.TILE, R.fuse_bound(radius), R.launches(radius, passes))
            assert p["fused"] == min(passes, p["fuse_bound"]) and p["launches"] == -(-passes // p["fused"])
    plans = [K.plan(c[3], c[4]) for c in R.cases()]
    assert sum(p["launches"] == 1 and p["fused"] > 1 for p in plans) >= 16
    assert sum(p["launches"] > 1 for p in plans) >= 16
    assert {p["launches"] for p in plans} >= {1, 2, 3}


def test_a_second_call_plane_forms_and_two_streams():
    """A call after another with other contents equals its own restatement, whatever the first left in the workspace; an (h, w)
    plane; uint16 tensors; two streams; the scene of the CPU test under the defaults"""
    top = 10000
    noisy, _ = R.scene(top)
    other = R.plane(1, 96, 128, "random", top)[0]
    for f, kw in ((K.Smoother(), {}), (K.Smoother(4, 3, 0.8, 5, 0.01, False), dict(radius=4, passes=3, sigma=0.8, A=5, Rq=655, pairs=False))):
        first = f(_codes_dev(other), top)
        want, stats = R.smooth(noisy[None], **kw)
        got, counts = f(_codes_dev(noisy), top, stats=True)
        assert got.shape == (96, 128) and got.dtype == torch.int16 and counts.shape == (1, 4)
        assert np.array_equal(_bits(got), want[0]) and np.array_equal(_bits(counts), stats)
        assert np.array_equal(_bits(first), R.smooth(other[None], **kw)[0][0])
        u16 = f(_codes_dev(noisy).view(torch.uint16), top)
        assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want[0])
        dev = _codes_dev(noisy)
        torch.cuda.synchronize()
        outs = []
        for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
            with torch.cuda.stream(stream):
                outs.append(f(dev, top, stats=True))
        torch.cuda.synchronize()
        for out, c in outs:
            assert np.array_equal(_bits(out), want[0]) and np.array_equal(_bits(c), stats)
    with pytest.raises(RuntimeError, match="smooth_depth expects"):
        f(dev.float(), top)
    with pytest.raises(ValueError, match="smooth_depth: depth_max 10000 with 8-bit codes"):
        f(dev.to(torch.uint8), top)
    with pytest.raises(ValueError, match="smooth_depth: tolerance 5 above the largest code 4"):
        f(dev, 4)


@pytest.mark.parametrize("radius, passes", [(2, 2), (4, 3)])
def test_capture_and_replay(radius, passes):
    """One call inside a capture (a single branch: the launches in a row on the capture's stream, no synchronisation) and one replay
    onto fresh contents of the same input tensor equal the eager call.  (4, 3) is a call of several launches wherever the rule splits
    it: its intermediate planes live in the per-stream workspace, which is allocated under the capture and held, so the case runs"""
    top = 65535
    f = K.Smoother(radius, passes, tolerance=40)
    a, b = _codes_dev(R.plane(3, 67, 67, "random", top)), _codes_dev(R.plane(3, 67, 67, "all", top))
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
    want, stats = R.smooth(R.plane(3, 67, 67, "all", top), radius, passes, None, 40, RQ, True)
    assert np.array_equal(_bits(out), want) and np.array_equal(_bits(counts), stats) and stats[:, 1].min() > 1000


@pytest.mark.parametrize("top", [255, 10000])
def test_planes_one_element_into_larger_buffers(top):
    """src, out and the workspace's neighbours: the planes one element into larger buffers (u8: an odd address; u16: two bytes off
    every wider alignment); the elements before and behind stay as they were"""
    lib = L.load()
    B, h, w = 2, 33, 65
    n = B * h * w
    c = R.plane(B, h, w, "random", top)
    want, stats = R.smooth(c, 4, 3, 0.8, 2, RQ, True)
    dt = torch.uint8 if top == 255 else torch.int16
    src = torch.full((n + 2,), 77, dtype=dt, device="cuda")
    src[1:n + 1] = _codes_dev(c).reshape(-1)
    out = torch.full((n + 2,), 99, dtype=dt, device="cuda")
    counts = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    tab = torch.from_numpy(K.weight_table(4, 0.8)).cuda()
    ws = torch.full((lib.codon_smooth_workspace_bytes(B, h, w) + 32,), 55, dtype=torch.uint8, device="cuda")
    e = src.element_size()
    call = smooth_caller(lib, src.data_ptr() + e, out.data_ptr() + e, tab.data_ptr(), counts.data_ptr(), ws.data_ptr() + 16, ws.numel() - 32,
                         ops._stream(torch.device("cuda:0")))
    st, msg = call(B=B, h=h, w=w, fmt=L.FILL_U8 if top == 255 else L.FILL_U16, top=top, radius=4, passes=3)
    assert st == 0, msg
    torch.cuda.synchronize()
    assert np.array_equal(_bits(out[1:n + 1]).reshape(B, h, w), want) and np.array_equal(_bits(counts), stats)
    assert out[0] == 99 and out[n + 1] == 99 and src[0] == 77 and src[n + 1] == 77
    assert (ws[:16] == 55).all() and (ws[-16:] == 55).all()


def test_refusals_leave_out_untouched():
    lib = L.load()
    c = R.plane(1, 5, 7, "random", 65535)
    src = _codes_dev(c)
    out = torch.full((2, 5, 7), -21555, dtype=torch.int16, device="cuda")
    counts = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    tab = torch.from_numpy(K.weight_table(2)).cuda()
    ws = torch.empty(256, dtype=torch.uint8, device="cuda")
    keep = src.clone()
    call = smooth_caller(lib, src.data_ptr(), out.data_ptr(), tab.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
                         ops._stream(torch.device("cuda:0")))
    smooth_refusals(lib, call)
    assert "unaligned" in call(src=src.data_ptr() + 1)[1] and "unaligned" in call(counts=counts.data_ptr() + 2)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and (counts == -7).all() and torch.equal(src, keep)
    assert call()[0] == 0                                             # and the good call goes through
    want, st = R.smooth(c)
    assert np.array_equal(_bits(out[:1]), want) and (out[1] == -21555).all()
    assert np.array_equal(_bits(counts[:1]), st) and (counts[1] == -7).all()


# ---- the command lines --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_and_register_smooth_write_the_bytes_of_the_commands_in_a_row(tmp_path, capsys, bits, top):
    """smooth.main on a two-file directory writes the restatement's PNGs and prints the statistics; `register --clean --smooth` on
    the sensor's files writes the bytes of clean, smooth and register run as separate commands, and prints their lines joined;
    without --smooth register's bytes and lines are what they are without this step"""
    shape = G.SHAPES[5]                                               # 70 x 130 onto 35 x 65 at scale 4 of 140 x 260
    hs, ws = shape[1:3]
    sensor, cleaned, smoothed, lr, chained, plain, only = (str(tmp_path / n) for n in ("sensor", "cleaned", "smoothed", "lr", "chained",
                                                                                        "plain", "only"))
    os.makedirs(sensor)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(G.calibration(shape, "mixed")))
    write = io.write_gray if bits == 8 else io.write_depth16
    c = R.plane(2, hs, ws, "random", top)
    names = ["a.png", "b.png"]
    for name, frame in zip(names, c):
        write(os.path.join(sensor, name), frame)
    fmt = ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []
    params = ["--radius", "3", "--passes", "3", "--sigma", "1.5", "--tolerance", "3", "--no-pairs"]
    capsys.readouterr()
    assert K.main(["--depth", sensor, "--out", only, "--stats", *params, *fmt]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    want, stats = R.smooth(c, 3, 3, 1.5, 3, RQ, False)
    for i, name in enumerate(names):
        got = io.read_depth_plane(os.path.join(only, name), bits, top)
        assert got.dtype == want.dtype and np.array_equal(got, want[i]), i
        v, ch, al, mx = (int(x) for x in stats[i])
        assert lines[i] == f"{name} valid={v} changed={ch} alone={al} max={mx}"
    assert stats[:, 1].min() > 0
    assert K.main(["--depth", sensor, "--out", str(tmp_path / "quiet"), *fmt]) == 0
    assert capsys.readouterr().out.strip().splitlines() == names
    # the three commands in a row
    reg = ["--calib", str(rig), "--scale", "4", "--depth-unit", repr(G.unit_of(top)), "--stats", *fmt]
    assert clean.main(["--depth", sensor, "--out", cleaned, "--stats", *fmt]) == 0
    clean_lines = capsys.readouterr().out.strip().splitlines()
    assert K.main(["--depth", cleaned, "--out", smoothed, "--stats", *params, *fmt]) == 0
    smooth_lines = capsys.readouterr().out.strip().splitlines()
    assert P.main(["--depth", smoothed, "--out", lr, *reg]) == 0
    reg_lines = capsys.readouterr().out.strip().splitlines()
    # and the one command
    assert P.main(["--depth", sensor, "--out", chained, "--clean", "--smooth", *("--smooth-" + p[2:] if p.startswith("--") else p for p in params),
                   *reg]) == 0
    got_lines = capsys.readouterr().out.strip().splitlines()
    for i, name in enumerate(names):
        assert open(os.path.join(chained, name), "rb").read() == open(os.path.join(lr, name), "rb").read(), name
        assert got_lines[i] == (reg_lines[i] + " cleaned: " + clean_lines[i].split(" ", 1)[1] + " smoothed: " + smooth_lines[i].split(" ", 1)[1])
    assert io.read_depth_plane(os.path.join(lr, names[0]), bits, top).shape == (35, 65)
    # without --smooth: the bytes of clean and register alone, and no word of the smoothing
    assert P.main(["--depth", sensor, "--out", plain, "--clean", *reg]) == 0
    plain_lines = capsys.readouterr().out.strip().splitlines()
    assert all("smoothed" not in ln and " cleaned: " in ln for ln in plain_lines)
    assert P.main(["--depth", cleaned, "--out", str(tmp_path / "ref"), *reg]) == 0
    ref_lines = capsys.readouterr().out.strip().splitlines()
    for i, name in enumerate(names):
        assert open(os.path.join(plain, name), "rb").read() == open(os.path.join(str(tmp_path / "ref"), name), "rb").read(), name
        assert plain_lines[i] == ref_lines[i] + " cleaned: " + clean_lines[i].split(" ", 1)[1]
    assert any(open(os.path.join(plain, n), "rb").read() != open(os.path.join(chained, n), "rb").read() for n in names)
