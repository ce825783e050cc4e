"""The triangle meshes of depth maps without a GPU: the numpy restatement tests/mesh_ref.py against what the definition
promises -- every branch of the triangle rule occurs over the shared patterns, the counts of patterns whose meshes are known, the
winding against the cloud's positions and normals -- and the host functions of codon_amd.cloud: the PLY header, writer and reader
with faces, the refusals of codon_cloud_mesh (on the host, before any HIP call) and of the command line."""
import ctypes as C
import re

import numpy as np
import pytest

from codon_amd import _lib as L
from codon_amd import cloud as K
from tests import cloud_ref as R
from tests import mesh_ref as M


# ---- the definition ------------------------------------------------------------------------------------------------------------------

def _kinds():
    """over the shared cases but the largest plane's: kind of quad -> [how many triangles the quads of that kind emit]"""
    seen = {}
    for shape in M.SHAPES[3:9]:
        for pattern, tol in M.cases(shape):
            for c in M.plane(shape, pattern):
                _, ok, kind = M.quad_faces(c, M.tolerance_of(tol, M.top_of(pattern)), M.RQ)
                for k in np.unique(kind):
                    seen.setdefault(int(k), set()).update(int(v) for v in np.unique(ok[kind == k].sum(axis=1)))
    return seen


def test_the_patterns_reach_every_branch_of_the_rule():
    """Both diagonals, a tie, each of the four three-corner triangles, a quad of four that emits exactly one triangle, quads that
    emit none -- with four corners, with three and with fewer"""
    seen = _kinds()
    assert 2 in seen[4] and 2 in seen[5] and 2 in seen[6]             # a-d, a tie, b-c: both triangles
    for missing in (M.A_, M.B_, M.C_, M.D_):
        assert seen[missing] >= {0, 1}, missing                       # the one candidate, emitted and refused
    assert 1 in seen[4] | seen[5] | seen[6] and 0 in seen[4] | seen[5] | seen[6]
    assert seen[-1] == {0}


def test_the_two_new_patterns():
    """holes: isolated single holes, every one of the four three-corner kinds; saddle: both diagonals and ties, all linked"""
    shape = M.SHAPES[8]
    c = M.plane(shape, "holes")[0]
    tri, ok, kind = M.quad_faces(c, 2, M.RQ)
    assert all((kind == m).sum() > 100 for m in range(4)) and not (kind == -1).any()
    assert (ok[kind < 4].sum(axis=1) == 1).all()                      # a quad around a hole: its one candidate
    assert (ok[kind >= 4].sum(axis=1) >= 1).all() and (ok[kind >= 4].sum(axis=1) == 1).sum() > 100      # around a flying pixel: one
    s = M.plane(shape, "saddle")[0]
    assert (s != 0).all() and int(s.max()) - int(s.min()) <= M.SADDLE_DELTA + 3
    tri, ok, kind = M.quad_faces(s, 2, M.RQ)
    assert min((kind == 4).sum(), (kind == 5).sum(), (kind == 6).sum()) > 100 and ok.all()
    # the tie takes a-d: (a, c, d) then (a, d, b)
    q = int(np.flatnonzero(kind == 5)[0])
    assert tri[q].tolist() == [[M.A_, M.C_, M.D_], [M.A_, M.D_, M.B_]]
    q = int(np.flatnonzero(kind == 6)[0])
    assert tri[q].tolist() == [[M.A_, M.C_, M.B_], [M.B_, M.C_, M.D_]]


def test_one_quad_by_hand():
    """The rule on 2 x 2 planes written out: vertex indices are ranks in row-major order"""
    f = lambda rows, A=2: M.faces_plane(np.array(rows, dtype=np.uint16), A, 0).tolist()      # noqa: E731
    assert f([[10, 11], [11, 12]]) == [[0, 2, 1], [1, 2, 3]]          # |a - d| = 2 > |b - c| = 0: b-c
    assert f([[10, 11], [12, 10]]) == [[0, 2, 3], [0, 3, 1]]          # |a - d| = 0 < 1: a-d
    assert f([[10, 11], [11, 10]]) == [[0, 2, 3], [0, 3, 1]]          # a tie: a-d
    assert f([[10, 11], [12, 0]]) == [[0, 2, 1]] and f([[0, 11], [12, 10]]) == [[0, 1, 2]]            # d, a missing
    assert f([[10, 0], [12, 10]]) == [[0, 1, 2]] and f([[10, 11], [0, 10]]) == [[0, 2, 1]]            # b, c missing: ranks shift
    assert f([[10, 0], [0, 10]]) == [] and f([[0, 0], [0, 0]]) == []
    assert f([[10, 11], [12, 90]]) == [[0, 2, 1]]                     # b-c; (b, c, d) fails its links, (a, c, b) stands alone
    assert f([[10, 13], [10, 10]]) == [[0, 2, 3]]                     # a-d; (a, d, b) fails: b is 3 away
    assert f([[10, 13], [13, 10]]) == []                              # a tie takes a-d, both triangles fail, b-c is not retried
    assert f([[10, 13], [13, 10]], 3) == [[0, 2, 3], [0, 3, 1]]
    # A is for one step, the same for sides and diagonals, and Rq adds a fraction of the smaller code
    assert f([[100, 102], [102, 104]]) == [[0, 2, 1], [1, 2, 3]] and f([[100, 102], [102, 105]]) == [[0, 2, 1]]
    assert M.faces_plane(np.array([[100, 102], [102, 105]], dtype=np.uint16), 2, 656).tolist() == [[0, 2, 1], [1, 2, 3]]   # + (656 * 102) >> 16 = 1
    assert M.records(np.array([[0, 2, 1]], dtype=np.int32)) == b"\x03" + b"\x00\x00\x00\x00\x02\x00\x00\x00\x01\x00\x00\x00"


@pytest.mark.parametrize("shape", M.SHAPES[:9], ids=lambda s: "x".join(map(str, s)))
def test_patterns_whose_meshes_are_known(shape):
    B, h, w = shape
    quads = (h - 1) * (w - 1)
    for tol in M.TOLERANCES:
        bodies, counts = M.want(shape, "all", tol)
        assert counts.tolist() == [2 * quads] * B and all(len(b) == M.row_bytes(h, w) for b in bodies)
        v = np.frombuffer(bodies[0], dtype=M.RECORD)
        assert (v["n"] == 3).all() and (quads == 0 or (v["v"].min() == 0 and v["v"].max() == h * w - 1))
        for pattern in ("checker", "none", "last"):
            assert M.want(shape, pattern, tol)[1].tolist() == [0] * B, (pattern, tol)
    for pattern in M.PATTERNS:                                        # every index is a vertex of the image's own cloud
        codes = M.plane(shape, pattern)
        for tol in M.TOLERANCES:
            bodies, counts = M.want(shape, pattern, tol)
            for b in range(B):
                v = np.frombuffer(bodies[b], dtype=M.RECORD)["v"]
                assert len(v) == counts[b] and (len(v) == 0 or (v.min() >= 0 and v.max() < (codes[b] != 0).sum()))
    for tol in ("zero", "default"):                                   # a foreground and a background are never joined
        c = M.plane(shape, "surfaces")[0]
        col = np.nonzero(c)[1]                                        # the column of every vertex
        v = np.frombuffer(M.want(shape, "surfaces", tol)[0][0], dtype=M.RECORD)["v"]
        side = col[v] < w // 2
        assert (side.all(axis=1) | (~side).all(axis=1)).all()
        assert len(v) == 2 * (h - 1) * max(w - 2, 0)                  # all but the column of quads across the edge
    if quads:
        assert M.want(shape, "surfaces", "top")[1][0] == 2 * quads    # the tolerance `top` joins them: the rule is what the test is about


def test_shapes_sit_on_the_run_edges():
    runs = lambda s: -(-(s[1] - 1) * (s[2] - 1) // M.RUN)            # noqa: E731
    assert [runs(s) for s in M.SHAPES] == [0, 0, 0, 1, 1, 1, 2, 1, 11, 259]
    assert (M.SHAPES[5][1] - 1) * (M.SHAPES[5][2] - 1) == M.RUN and (M.SHAPES[6][1] - 1) * (M.SHAPES[6][2] - 1) == M.RUN + 1
    assert runs(M.BIG) > 256                                          # a thread of the scan takes more than one word
    n = sum(len(M.cases(s)) for s in M.SHAPES)
    assert n == 9 * len(M.PATTERNS) * len(M.TOLERANCES) + len(M.BIG_CASES) == 274
    # the spans of the runs of one case start at all four addresses modulo 4, one byte into a buffer
    c = M.plane(M.SHAPES[8], "random")[0]
    _, ok, _ = M.quad_faces(c, 2, M.RQ)
    per = ok.sum(axis=1)
    starts = np.concatenate([[0], np.cumsum([per[q:q + M.RUN].sum() for q in range(0, per.size, M.RUN)])[:-1]])
    assert {int((1 + s * M.REC) % 4) for s in starts} == {0, 1, 2, 3}


@pytest.mark.parametrize("top, z0", [(10000, 2000), (65535, 20000)])
def test_faces_face_the_camera(top, z0):
    """On the slanted plane every face's geometric normal, from the float positions of the cloud, points towards the camera
    (a negative dot product with the centroid) and to the side of each of its vertices' normals"""
    c, _ = R.slanted_plane(top, z0)
    rx, ry = R.ray_tables(60, 40, 500.0, 500.0, 29.5, 19.5)
    rec, counts, _ = R.cloud_plane(c, rx, ry, tolerance=max(2, top // 500))
    f = M.faces_plane(c, 2, M.RQ)
    assert len(f) == 2 * 39 * 59 and counts[1] == counts[0] == 40 * 60
    P = np.stack([rec[n] for n in "xyz"], axis=1).astype(np.float64)
    N = np.stack([rec[n] for n in ("nx", "ny", "nz")], axis=1).astype(np.float64)
    g = np.cross(P[f[:, 1]] - P[f[:, 0]], P[f[:, 2]] - P[f[:, 0]])
    assert ((g * P[f].mean(axis=1)).sum(axis=1) < 0).all() and (g[:, 2] < 0).all()
    for q in range(3):
        assert ((g * N[f[:, q]]).sum(axis=1) > 0).all()


def test_int16_view_is_read_as_unsigned():
    c = M.plane(M.SHAPES[7], "high")[0]
    assert (c >= 32768).sum() > 100
    assert np.array_equal(M.faces_plane(c, 2, M.RQ), M.faces_plane(c.view(np.int16), 2, M.RQ)) and len(M.faces_plane(c, 2, M.RQ)) > 50


# ---- the host functions ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("normals", [False, True])
@pytest.mark.parametrize("color", [False, True])
def test_mesh_round_trip_and_header_bytes(tmp_path, normals, color):
    shape = M.SHAPES[4]
    rx, ry = R.ray_tables(shape[2], shape[1], 9.0, 9.0, 3.0, 2.0)
    c = M.plane(shape, "holes")[0]
    rec, counts, _ = R.cloud_plane(c, rx, ry, normals=normals, color=R.tint(shape, 3)[0] if color else None)
    faces = M.faces_plane(c, 2, M.RQ)
    n, F = len(rec), len(faces)
    assert F > 10
    vertex = ("ply\nformat binary_little_endian 1.0\ncomment x right, y down, z forward, in metres\n" + f"element vertex {n}\n"
              + "property float x\nproperty float y\nproperty float z\n"
              + ("property float nx\nproperty float ny\nproperty float nz\n" if normals else "")
              + ("property uchar red\nproperty uchar green\nproperty uchar blue\n" if color else ""))
    # without faces every byte is what it was
    assert K.ply_header(n, normals, color) == K.ply_header(n, normals, color, None) == (vertex + "end_header\n").encode("ascii")
    head = K.ply_header(n, normals, color, F)
    assert head == (vertex + f"element face {F}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert K.FACE_REC == M.REC and K.FACE_DTYPE == M.RECORD
    path = str(tmp_path / "a.ply")
    K.write_ply(path, rec.tobytes() + b"\xee" * 40, n, normals, color, M.records(faces) + b"\xee" * 30, F)      # prefixes are written
    with open(path, "rb") as fh:
        assert fh.read() == head + rec.tobytes() + M.records(faces)
    v, f = K.read_mesh(path)
    assert v.dtype == rec.dtype and v.tobytes() == rec.tobytes() and f.dtype == np.int32 and np.array_equal(f, faces)
    K.write_ply(path, rec.tobytes(), n, normals, color, np.frombuffer(M.records(faces), dtype=np.uint8), F)
    assert np.array_equal(K.read_mesh(path)[1], faces)
    K.write_ply(path, rec.tobytes(), n, normals, color, b"", 0)      # a mesh without a face is a mesh
    v, f = K.read_mesh(path)
    assert len(v) == n and f.shape == (0, 3)
    with pytest.raises(ValueError, match="not the header codon_amd.cloud writes"):
        K.read_ply(path)                                              # read_ply stays as it is: a cloud's header alone
    K.write_ply(path, rec.tobytes(), n, normals, color)              # and without faces the file is the cloud's
    with open(path, "rb") as fh:
        assert fh.read() == K.ply_header(n, normals, color) + rec.tobytes()
    assert K.read_ply(path).tobytes() == rec.tobytes()
    with pytest.raises(ValueError, match="read_mesh: .* names no vertex count or no face count"):
        K.read_mesh(path)
    with pytest.raises(ValueError, match="write_ply: .* bytes of faces"):
        K.write_ply(path, rec.tobytes(), n, normals, color, M.records(faces)[:-1], F)
    with pytest.raises(ValueError, match="write_ply: face_count 3 without faces"):
        K.write_ply(path, rec.tobytes(), n, normals, color, None, 3)
    with open(path, "wb") as fh:
        fh.write(head + rec.tobytes() + M.records(faces)[:-1])
    with pytest.raises(ValueError, match="read_mesh: .* bytes of body"):
        K.read_mesh(path)
    with open(path, "wb") as fh:
        fh.write(head + rec.tobytes() + b"\x04" + M.records(faces)[1:])
    with pytest.raises(ValueError, match="a face that is no triangle"):
        K.read_mesh(path)
    with open(path, "wb") as fh:
        fh.write(b"P6\n1 1\n255\n")
    with pytest.raises(ValueError, match="read_mesh: .* is not a PLY file"):
        K.read_mesh(path)
    with pytest.raises(ValueError, match="ply_header: faces -1"):
        K.ply_header(n, normals, color, -1)


def mesh_caller(lib, src, faces, counts, ws, stream=None):
    """The good call of mesh_ref.REFUSALS -- u16 codes, a 5 x 7 plane -- over the given addresses, with what a refusal changes as
    keyword arguments; shared with the GPU test"""
    P_ = C.c_void_p

    def call(B=1, h=5, w=7, src=src, fmt=L.FILL_U16, top=65535, tol_abs=2, tol_rel=M.RQ, faces=faces, counts=counts, ws=ws, ws_bytes=None):
        need = lib.codon_cloud_mesh_workspace_bytes(B, h, w)
        ws_bytes = need if ws_bytes is None else need - 1
        p = lambda v: None if v is None else P_(v)                    # noqa: E731
        st = lib.codon_cloud_mesh(B, h, w, p(src), fmt, top, tol_abs, tol_rel, p(faces), p(counts), p(ws), ws_bytes, stream)
        return st, lib.codon_last_error_string().decode()
    return call


def mesh_refusals(lib, call):
    for kw, word in M.REFUSALS:
        st, msg = call(**kw)
        assert st == -1 and msg.startswith("cloud_mesh: ") and word in msg, (kw, msg)
        with pytest.raises(RuntimeError, match="cloud_mesh failed with status -1: cloud_mesh: "):
            L.check(st, "cloud_mesh")


def test_c_entry_refusals_without_gpu():
    lib = L.load()
    q = lib.codon_cloud_mesh_workspace_bytes
    # block words, run words, the scan's two counts, the index plane: each rounded up to 16 bytes
    assert q(1, 5, 7) == 16 + 16 + 16 + 4 * 36 and q(3, 5, 7) == 48 + 48 + 32 + 4 * 108 and q(1, 33, 33) == 16 + 16 + 16 + 4 * 1092
    assert q(1, 26, 42) == 16 + 16 + 16 + 4 * 1092 and q(1, 520, 512) == 4 * (260 + 260 + 4 + 520 * 512)
    assert q(1, 1, 37) == 16 + 16 + 16 + 4 * 40 and q(1, 37, 1) > 0 and q(1, 1, 1) > 0             # no quad: accepted, not refused
    assert q(1, 4096, 4096) == 4 * (16384 + 16380 + 4 + 4096 * 4096)
    assert q(0, 5, 7) == 0 and q(65536, 5, 7) == 0 and q(1, 0, 7) == 0 and q(1, 5, 4097) == 0
    call = mesh_caller(lib, 4096, 8193, 12288, 16384)                 # never dereferenced: every call is refused on the host
    mesh_refusals(lib, call)
    for kw in ({"src": 4097}, {"counts": 12290}, {"ws": 16392}):
        assert "unaligned" in call(**kw)[1], kw
    # the faces need no alignment, and at the bounds themselves the refusal is the short workspace
    assert "too small" in call(top=10000, tol_abs=10000, tol_rel=65535, ws_bytes="short")[1]
    assert "too small" in call(fmt=L.FILL_U8, top=255, tol_abs=0, tol_rel=0, src=4097, ws_bytes="short")[1]
    # a plane without a quad has no face, and its face buffer may be null
    assert "too small" in call(h=1, faces=None, ws_bytes="short")[1] and "too small" in call(w=1, faces=None, ws_bytes="short")[1]
    assert "null pointer" in call(h=2, w=2, faces=None)[1]


# ---- the command line ---------------------------------------------------------------------------------------------------------------

NEEDED = ["--depth", "d", "--calib", "c.json", "--out", "o"]


def test_command_line_mesh_options(capsys):
    a, _ = K.parse_args(NEEDED)
    assert not a.mesh and (a.mesh_tolerance, a.mesh_tolerance_rel) == (2, 0.02)
    a, _ = K.parse_args([*NEEDED, "--mesh"])
    assert a.mesh and (a.mesh_tolerance, a.mesh_tolerance_rel) == (2, 0.02) == (K.DEFAULTS["tolerance"], K.DEFAULTS["tolerance_rel"])
    a, _ = K.parse_args([*NEEDED, "--mesh", "--no-normals", "--mesh-tolerance", "0", "--mesh-tolerance-rel", "0.5"])
    assert a.mesh and a.no_normals and (a.mesh_tolerance, a.mesh_tolerance_rel) == (0, 0.5)
    for argv, word in (([*NEEDED, "--mesh-tolerance", "2"], "--mesh-tolerance without --mesh"),
                       ([*NEEDED, "--mesh-tolerance-rel", "0.02"], "--mesh-tolerance-rel without --mesh"),
                       ([*NEEDED, "--mesh", "--mesh-tolerance", "-1"], "--mesh-tolerance -1 must be in \\[0, 255\\]"),
                       ([*NEEDED, "--mesh", "--mesh-tolerance", "256"], "--mesh-tolerance 256 must be in \\[0, 255\\]"),
                       ([*NEEDED, "--mesh", "--depth-bits", "16", "--depth-max", "10000", "--mesh-tolerance", "10001"],
                        "--mesh-tolerance 10001 must be in \\[0, 10000\\]"),
                       ([*NEEDED, "--mesh", "--mesh-tolerance-rel", "1.0"], "--mesh-tolerance-rel 1.0 must be in \\[0, 1\\)")):
        with pytest.raises(SystemExit) as e:
            K.parse_args(argv)
        assert e.value.code == 2 and re.search(word, capsys.readouterr().err), argv
    assert "untuned" in K.__doc__ and "--mesh" in K.__doc__
