"""The triangle meshes of depth maps on the MI355X against the numpy restatement tests/mesh_ref.py (pinned on the CPU by
tests/test_mesh_cpu.py).  The bar is EQUAL BYTES, faces and counts, no tolerance anywhere.
Shapes (mesh_ref.SHAPES), the smallest at which each part can go wrong: three planes without a quad; one quad; a small plane;
exactly one run of 1024 quads; a second run that holds one quad; a batch of three, for the per-image offsets; 93 x 116, many runs
whose spans start at every address modulo 4 and whose rows are not aligned; 520 x 512, 259 runs, so a thread of the scan takes more
than one run word.  Every shape under every pattern -- u8, u16 and the codes of 32768 and above among them -- and the tolerances 0,
the default and `top` (mesh_ref.cases; four of them on the largest).  In every case the codes and the faces each start one element,
or one byte, into a larger buffer -- the staged 4-byte stores run on an odd base address -- and the buffer is prefilled: nothing
before its first byte and nothing behind its last is written; what lies behind counts[b] * 13 bytes of a row is not compared."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import cloud as K
from codon_amd import io, ops
from codon_amd import register as P
from tests import cloud_ref as R
from tests import mesh_ref as M
from tests.test_mesh_cpu import mesh_caller, mesh_refusals

pytestmark = pytest.mark.gpu

ids = lambda s: "x".join(map(str, s))                                # noqa: E731
FILL = 0xA7


def _stream():
    return ops._stream(torch.device("cuda:0"))


def _codes(a):
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)


class Raw:
    """One case through the C entry, the codes and the faces one element into larger buffers"""

    def __init__(self, shape, pattern, tol):
        self.shape, self.pattern, self.tol = shape, pattern, tol
        B, h, w = shape
        self.top = M.top_of(pattern)
        self.A = M.tolerance_of(tol, self.top)
        codes = _codes(M.plane(shape, pattern)).reshape(-1)
        self.codes_buf = torch.full((codes.numel() + 2,), 1, dtype=codes.dtype, device="cuda")
        self.codes = self.codes_buf[1:-1]
        self.codes.copy_(codes.cuda())
        self.n = B * M.row_bytes(h, w)
        self.faces = torch.full((self.n + 2,), FILL, dtype=torch.uint8, device="cuda")
        self.counts = torch.full((B,), -7, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(L.load().codon_cloud_mesh_workspace_bytes(B, h, w), dtype=torch.uint8, device="cuda")

    def run(self, stream=None):
        B, h, w = self.shape
        P_ = C.c_void_p
        st = L.load().codon_cloud_mesh(B, h, w, P_(self.codes.data_ptr()), L.FILL_U8 if self.top == 255 else L.FILL_U16, self.top, self.A,
                                       M.RQ, P_(self.faces.data_ptr() + 1), P_(self.counts.data_ptr()), P_(self.ws.data_ptr()),
                                       self.ws.numel(), _stream() if stream is None else stream)
        L.check(st, "cloud_mesh")

    def check(self, pattern=None):
        """the counts and the first counts[b] * 13 bytes of every row against the restatement of `pattern` (the object's own if None)"""
        B, h, w = self.shape
        bodies, counts = M.want(self.shape, pattern or self.pattern, self.tol)
        what = (self.shape, pattern or self.pattern, self.tol)
        torch.cuda.synchronize()
        assert np.array_equal(self.counts.cpu().numpy().view(np.uint32), counts), (what, self.counts.tolist(), counts.tolist())
        got = self.faces.cpu().numpy()
        assert got[0] == FILL and got[-1] == FILL, (what, "a byte outside the faces was written")
        got = got[1:-1].reshape(B, M.row_bytes(h, w))
        for b, body in enumerate(bodies):
            want = np.frombuffer(body, dtype=np.uint8)
            bad = np.flatnonzero(got[b, :len(want)] != want)
            assert bad.size == 0, f"{what} image {b}: {bad.size} bytes differ, the first in face {bad[0] // M.REC} at byte {bad[0] % M.REC}"
        assert self.codes_buf[0] == 1 and self.codes_buf[-1] == 1


@pytest.mark.parametrize("shape", M.SHAPES, ids=ids)
def test_equals_the_restatement(shape):
    """mesh_ref.cases: every pattern under the tolerances 0, the default and top; u8, u16 and codes of 32768 and above"""
    for pattern, tol in M.cases(shape):
        if pattern == "high":
            assert (M.plane(shape, pattern).view(np.int16) < 0).sum() > 0               # as an int16 view, negative
        case = Raw(shape, pattern, tol)
        case.run()
        case.check()


def test_a_second_call_the_python_interface_and_the_clouds_vertices():
    """The workspace is initialised by every call: a second call on the same buffers with other codes equals its own restatement.
    triangulate gives the same bytes, for (h, w) planes and uint16 tensors too, and every index is below the number of points
    Unprojection gives for the same codes"""
    shape = M.SHAPES[8]
    case = Raw(shape, "all", "default")
    case.run()
    case.check()
    for pattern in ("random", "none", "holes", "random"):
        case.codes.copy_(_codes(M.plane(shape, pattern)).reshape(-1).cuda())
        case.run()
        case.check(pattern)
    shape = M.SHAPES[7]
    un = K.Unprojection(P.Camera(shape[2], shape[1], *R.camera_of(shape)))
    for pattern in ("random", "holes", "surfaces"):
        codes = _codes(M.plane(shape, pattern)).cuda()
        got = K.triangulate(codes, depth_max=10000)
        bodies, counts = M.want(shape, pattern, "default")
        assert got.body.shape == (shape[0], M.row_bytes(*shape[1:])) and got.body.dtype == torch.uint8 and got.counts.dtype == torch.int32
        assert np.array_equal(got.counts.cpu().numpy().view(np.uint32), counts)
        points = un(codes, depth_max=10000).counts.cpu().numpy()[:, 0]
        for b, body in enumerate(bodies):
            raw = got.body[b, :len(body)].cpu().numpy()
            assert raw.tobytes() == body
            v = np.frombuffer(raw.tobytes(), dtype=M.RECORD)["v"]
            assert len(v) > 0 and v.min() >= 0 and v.max() < points[b], (pattern, b)
        one = K.triangulate(codes[1], depth_max=10000)
        u16 = K.triangulate(codes[1].view(torch.uint16), tolerance=2, tolerance_rel=0.02, depth_max=10000)
        for f in (one, u16):
            assert f.counts.tolist() == [int(counts[1])] and f.body[0, :len(bodies[1])].cpu().numpy().tobytes() == bodies[1]
    row = K.triangulate(_codes(M.plane(M.SHAPES[1], "all")).cuda())     # a plane without a quad: no face, and no byte
    assert row.body.shape == (1, 0) and row.counts.tolist() == [0]
    u8 = K.triangulate(_codes(M.plane(M.SHAPES[4], "u8")).cuda(), tolerance=0)
    assert u8.body[0, :len(M.want(M.SHAPES[4], "u8", "zero")[0][0])].cpu().numpy().tobytes() == M.want(M.SHAPES[4], "u8", "zero")[0][0]
    codes = _codes(M.plane(shape, "random")).cuda()
    with pytest.raises(RuntimeError, match="cloud_mesh expects"):
        K.triangulate(codes.float())
    with pytest.raises(ValueError, match="cloud_mesh: tolerance 20 above the largest code 5"):
        K.triangulate(codes, tolerance=20, depth_max=5)
    with pytest.raises(ValueError, match="cloud_mesh: tolerance -1 "):
        K.triangulate(codes, tolerance=-1)
    with pytest.raises(ValueError, match="cloud_mesh: tolerance_rel 1.0 "):
        K.triangulate(codes, tolerance_rel=1.0)


def test_refusals_leave_every_output_untouched():
    lib = L.load()
    case = Raw(M.SHAPES[4], "random", "default")
    keep = case.codes_buf.clone()
    call = mesh_caller(lib, case.codes.data_ptr(), case.faces.data_ptr() + 1, case.counts.data_ptr(), case.ws.data_ptr(), stream=_stream())
    mesh_refusals(lib, call)
    assert "unaligned" in call(src=case.codes.data_ptr() + 1)[1] and "unaligned" in call(ws=case.ws.data_ptr() + 8)[1]
    assert "unaligned" in call(counts=case.counts.data_ptr() + 2)[1]
    torch.cuda.synchronize()
    assert (case.faces == FILL).all() and (case.counts == -7).all() and torch.equal(case.codes_buf, keep)
    st, msg = call(top=10000)                                         # and the good call goes through
    assert st == 0, msg
    case.check()


# ---- the command line ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits, top", [(8, 255), (16, 10000)])
def test_main_writes_header_vertices_and_faces(tmp_path, capsys, bits, top):
    """cloud.main --mesh on a small directory: every file is exactly the header, cloud_ref's vertex bytes and mesh_ref's face bytes,
    with the statistics line; with --no-normals and other tolerances too; and the same run without --mesh writes exactly the header
    and cloud_ref's vertex bytes, line for line today's"""
    h, w = 37, 52
    cam = dict(width=w, height=h, fx=61.5, fy=60.25, cx=25.25, cy=18.5)
    rig = tmp_path / "rig.json"
    rig.write_text(json.dumps({"depth": cam, "color": cam, "rotation": np.eye(3).tolist(), "translation": [0.0, 0.0, 0.0]}))
    depth, out, plain, bare = (str(tmp_path / n) for n in ("depth", "out", "plain", "bare"))
    os.makedirs(depth)
    write = io.write_gray if bits == 8 else io.write_depth16
    planes = []
    for i, pattern in enumerate(("u8" if bits == 8 else "random", "holes", "surfaces")):
        c = np.clip(M.plane((1, h, w), pattern)[0], 0, top).astype(np.uint8 if bits == 8 else np.uint16)
        write(os.path.join(depth, f"{i:02d}.png"), c)
        planes.append(c)
    fmt = ["--depth-bits", "16", "--depth-max", str(top)] if bits == 16 else []
    base = ["--depth", depth, "--calib", str(rig), *fmt]
    rx, ry = R.ray_tables(w, h, cam["fx"], cam["fy"], cam["cx"], cam["cy"])
    capsys.readouterr()
    assert K.main([*base, "--out", out, "--mesh", "--stats"]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    assert K.main([*base, "--out", plain, "--stats"]) == 0
    plain_lines = capsys.readouterr().out.strip().splitlines()
    assert K.main([*base, "--out", bare, "--mesh", "--no-normals", "--mesh-tolerance", "0", "--mesh-tolerance-rel", "0.001"]) == 0
    assert capsys.readouterr().out.strip().splitlines() == ["00.png", "01.png", "02.png"]
    total = 0
    for i, c in enumerate(planes):
        rec, counts, _ = R.cloud_plane(c, rx, ry)
        faces = M.faces_plane(c, 2, M.RQ)
        with open(os.path.join(out, f"{i:02d}.ply"), "rb") as fh:
            assert fh.read() == K.ply_header(len(rec), True, False, len(faces)) + rec.tobytes() + M.records(faces), i
        assert lines[i] == f"{i:02d}.png points={counts[0]} normals={counts[1]} faces={len(faces)}"
        v, f = K.read_mesh(os.path.join(out, f"{i:02d}.ply"))
        assert v.tobytes() == rec.tobytes() and np.array_equal(f, faces)
        with open(os.path.join(plain, f"{i:02d}.ply"), "rb") as fh:
            assert fh.read() == K.ply_header(len(rec), True, False) + rec.tobytes(), i
        assert plain_lines[i] == f"{i:02d}.png points={counts[0]} normals={counts[1]}"
        xyz, _, _ = R.cloud_plane(c, rx, ry, normals=False)
        tight = M.faces_plane(c, 0, M.rel_q16(0.001))
        with open(os.path.join(bare, f"{i:02d}.ply"), "rb") as fh:
            assert fh.read() == K.ply_header(len(xyz), False, False, len(tight)) + xyz.tobytes() + M.records(tight), i
        total += len(faces)
    assert total > 1000
