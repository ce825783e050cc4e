"""The depth registration on the MI355X against the numpy restatement tests/register_ref.py (pinned on the CPU by
tests/test_register_cpu.py).  The bar is EQUAL BITS, codes and statistics, no tolerance anywhere: the z-buffer's minimum and the
counts do not depend on the order of the atomics.
Shapes (register_ref.SHAPES), the smallest at which each part can go wrong: one pixel onto one pixel; odd sizes; exactly one 16 x 16
tile of source pixels; one pixel past a tile on both axes onto a finer grid (footprints of 2 - 4, and up to 8 and beyond under the
near pattern); a batch of three onto a coarser grid (empty footprints, several pixels under one minimum); several tiles at scale 4
from a 140 x 260 colour image (2275 target pixels: three runs of the resolve launch, the last partial)."""
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops
from codon_amd import register as P
from tests import register_ref as G
from tests.test_register_cpu import register_caller, register_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s[:5]))                            # noqa: E731


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _bits(t):
    a = t.cpu().numpy()
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32}[a.dtype.itemsize])


@pytest.mark.parametrize("shape", G.SHAPES, ids=ids)
def test_equals_the_restatement(shape):
    """register_ref.cases: every pattern under every calibration, the formats in turn -- codes and statistics; no argument is
    modified; a call without statistics gives the same codes"""
    regs = {}
    seen = np.zeros(4, dtype=np.int64)
    for name, top, pattern, calib in G.cases(shape):
        key = (calib, top)
        if key not in regs:
            regs[key] = P.Registration(P.Calibration.from_mapping(G.calibration(shape, calib)), shape[5], G.unit_of(top))
            A, T, Q = G.tables(shape, calib, top)
            assert np.array_equal(regs[key].rays.cpu().numpy(), A) and np.array_equal(regs[key].trans, T)
            assert np.array_equal(regs[key].proj, Q) and regs[key].out_size == shape[3:5]
        reg = regs[key]
        want, stats = G.want(shape, pattern, top, calib)
        src = _codes_dev(G.plane(shape, pattern, top))
        before = src.clone()
        dm = None if top == 255 else top
        got, counts = reg(src, dm, stats=True)
        assert got.shape == want.shape and got.dtype == src.dtype and got.is_contiguous()
        assert counts.shape == (shape[0], 4) and counts.dtype == torch.int32
        bad = np.argwhere(_bits(got) != want)
        assert bad.size == 0, f"{shape} {name} {pattern} {calib}: {len(bad)} codes differ, first at {bad[:3].tolist()}"
        assert np.array_equal(_bits(counts), stats), (shape, name, pattern, calib, _bits(counts).tolist(), stats.tolist())
        assert torch.equal(reg(src, dm), got) and torch.equal(src, before)
        if pattern == "all":
            assert not got.any() and not counts.any()
        seen += stats.astype(np.int64).sum(axis=0)
    assert (seen > 0).all() or shape[1:3] == (1, 1)                  # every count counts something on every shape but the pixel


def test_a_second_call_and_plane_forms():
    """The workspace is initialised by every call: a second call on the same stream with another plane equals its own
    restatement, whatever the first left behind.  (h, w) planes, uint16 tensors, two streams with a workspace each."""
    shape, top = G.SHAPES[3], 10000
    reg = P.Registration(P.Calibration.from_mapping(G.calibration(shape, "mixed")), 1, G.unit_of(top))
    first = reg(_codes_dev(G.plane(shape, "none", top)), top)
    for pattern in ("random", "all", "scene", "none"):
        want, stats = G.want(shape, pattern, top, "mixed")
        got, counts = reg(_codes_dev(G.plane(shape, pattern, top)), top, stats=True)
        assert np.array_equal(_bits(got), want) and np.array_equal(_bits(counts), stats), pattern
    assert torch.equal(got, first)
    want, stats = G.want(shape, "random", top, "mixed")
    dev = _codes_dev(G.plane(shape, "random", top))
    one, c1 = reg(dev[0], top, stats=True)
    assert one.shape == (40, 80) and one.dtype == torch.int16 and np.array_equal(_bits(one), want[0]) and c1.shape == (1, 4)
    u16 = reg(dev.view(torch.uint16), top)
    assert u16.dtype == torch.uint16 and np.array_equal(_bits(u16.view(torch.int16)), want)
    torch.cuda.synchronize()
    outs = []
    for stream in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(stream):
            outs.append(reg(dev, top))
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and np.array_equal(_bits(outs[0]), want)
    with pytest.raises(ValueError, match="register_depth: a 17x32 plane, and the depth camera of the calibration is 17x33"):
        reg(dev[:, :, :32], top)
    with pytest.raises(RuntimeError, match="register_depth expects"):
        reg(dev.float(), top)
    with pytest.raises(ValueError, match="register_depth: depth_max 10000 with 8-bit codes"):
        reg(dev.to(torch.uint8), top)
    with pytest.raises(ValueError, match="depth_max 0 must be an integer"):
        reg(dev, 0)


def test_radial_files():
    shape, top = G.SHAPES[3], 65535
    m = G.calibration(shape, "mixed")
    d = m["depth"]
    A = G.ray_table(17, 33, d["fx"], d["fy"], d["cx"], d["cy"], d["dist"], m["rotation"], radial=True)
    _, T, Q = G.tables(shape, "mixed", top)
    c = G.plane(shape, "random", top)
    want, stats = G.register(c, A, T, Q, 40, 80, top)
    got, counts = P.Registration(P.Calibration.from_mapping(m), 1, G.unit_of(top), radial=True)(_codes_dev(c), stats=True)
    assert np.array_equal(_bits(got), want) and np.array_equal(_bits(counts), stats)
    assert not np.array_equal(want, G.want(shape, "random", top, "mixed")[0])


def test_capture_and_replay():
    """One call inside a capture (a single branch: three launches in a row on the capture's stream) and one replay equal the eager
    call; the replay runs on other contents of the same input tensor"""
    shape, top = G.SHAPES[5], 65535
    reg = P.Registration(P.Calibration.from_mapping(G.calibration(shape, "mixed")), 4, G.unit_of(top))
    a, b = _codes_dev(G.plane(shape, "random", top)), _codes_dev(G.plane(shape, "scene", top))
    eager = reg(b, stats=True)
    src = a.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, counts = reg(src, stats=True)
    src.copy_(b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager[0]) and torch.equal(counts, eager[1])
    want, stats = G.want(shape, "scene", top, "mixed")
    assert np.array_equal(_bits(out), want) and np.array_equal(_bits(counts), stats)


def test_refusals_leave_out_untouched():
    lib = L.load()
    shape = G.SHAPES[1]
    A, T, Q = G.tables(shape, "translation", 65535)
    src = _codes_dev(G.plane(shape, "random", 65535))
    rays = torch.from_numpy(A.copy()).cuda()
    ws = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 3, 5), -21555, dtype=torch.int16, device="cuda")
    stats = torch.full((2, 4), -7, dtype=torch.int32, device="cuda")
    keep = src.clone()
    call = register_caller(lib, src.data_ptr(), rays.data_ptr(), out.data_ptr(), ws.data_ptr(), stats.data_ptr(),
                           ops._stream(torch.device("cuda:0")))
    register_refusals(lib, call)
    assert "unaligned" in call(src=src.data_ptr() + 1)[1] and "unaligned" in call(ws=ws.data_ptr() + 8)[1]
    torch.cuda.synchronize()
    assert (out == -21555).all() and (stats == -7).all() and torch.equal(src, keep)
    assert call(T=tuple(int(v) for v in T), P=tuple(int(v) for v in Q))[0] == 0        # and the good call goes through
    want, st = G.want(shape, "random", 65535, "translation")
    assert np.array_equal(_bits(out[0]), want[0]) and (out[1] == -21555).all()
    assert np.array_equal(_bits(stats[0]), st[0]) and (stats[1] == -7).all()


# ---- the command line, and infer on what it wrote ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_writes_what_infer_reads(tmp_path, capsys, bits, top):
    """register.main on three files at scale 4 writes PNGs equal to the restatement and prints the statistics; infer --lr-depth
    --baseline bicubic --fill-holes then runs on them with the colour images: the composition, with no network needed"""
    shape = G.SHAPES[5]
    m = G.calibration(shape, "mixed")
    sensor, color, lr = (str(tmp_path / n) for n in ("sensor", "color", "lr"))
    os.makedirs(sensor), os.makedirs(color)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps(m))
    write = io.write_gray if bits == 8 else io.write_depth16
    A, T, Q = G.tables(shape, "mixed", top)
    g = np.random.default_rng(5)
    wants = []
    for i, pattern in enumerate(("random", "scene", "none")):
        c = G.plane(shape, pattern, top, seed=2 + i)[0]
        write(os.path.join(sensor, f"{i:02d}.png"), c)
        io.write_gray(os.path.join(color, f"{i:02d}.png"), g.integers(0, 256, size=(140, 260), dtype=np.uint8))
        wants.append(G.register_plane(c, A, T, Q, 35, 65, top))
    argv = ["--depth", sensor, "--calib", str(rig), "--out", lr, "--scale", "4", "--depth-unit", repr(G.unit_of(top))]
    argv += ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []
    capsys.readouterr()
    assert P.main(argv + ["--stats"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 3
    for i, (want, stats) in enumerate(wants):
        got = io.read_depth_plane(os.path.join(lr, f"{i:02d}.png"), bits, top)
        assert got.dtype == want.dtype and np.array_equal(got, want), i
        v, o, d, f = (int(x) for x in stats)
        assert lines[i] == f"{i:02d}.png valid={v} outside={o} dropped={d} filled={f}"
        assert (want == 0).any() and f > 0
    assert P.main(argv + ["--out", str(tmp_path / "quiet")]) == 0
    assert capsys.readouterr().out.strip().splitlines() == ["00.png", "01.png", "02.png"]
    sr = str(tmp_path / "sr")
    rc = infer.main(["--scale", "4", "--lr-depth", lr, "--input-color", color, "--out", sr, "--baseline", "bicubic", "--fill-holes"]
                    + (["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []))
    assert rc == 0
    up = io.read_depth_plane(os.path.join(sr, "01.png"), bits, top)
    assert up.shape == (140, 260) and (up != 0).all()
