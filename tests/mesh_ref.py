"""numpy restatement of the triangle meshes of depth maps (codon_amd/csrc/cloud.hip, mesh_tile.h, codon_amd.cloud.triangulate; DESIGN
12.22) and the inputs its tests share -- TEST INFRASTRUCTURE.  The kernels are held to these bytes, no tolerance.  A DEFINITION of
this project.

Vertices: the cloud's own.  The vertex index of a non-zero code is its rank among the non-zero codes of the plane in row-major
order: its position in the body codon_cloud_points writes (tests/cloud_ref.py).
Quads: quad (i, j), 0 <= i < h - 1, 0 <= j < w - 1, has the corners a = (i, j), b = (i, j + 1), c = (i + 1, j), d = (i + 1, j + 1),
codes k_a .. k_d.  Two corners are LINKED by clean_ref.linked(k1, k2, A, Rq) with A = tolerance for ONE step -- not multiplied, the
same for sides and diagonals -- and Rq = rel_q16(tolerance_rel); a hole links to nothing.  A triangle is emitted when its three
corners are pairwise linked.
  four non-zero corners   the diagonal is a-d if |k_a - k_d| <= |k_b - k_c| (a tie takes a-d) and b-c otherwise; a-d gives (a, c, d)
                          then (a, d, b), b-c gives (a, c, b) then (b, c, d); each of the two is emitted or not on its own, and the
                          other diagonal is not retried
  exactly three           one candidate: d missing (a, c, b); a missing (b, c, d); b missing (a, c, d); c missing (a, d, b)
  fewer                   no triangle
Winding: with x right, y down, z forward these orders give a geometric normal with negative z on a fronto-parallel surface --
towards the camera, the side the vertex normals face.
Faces go in row-major order of the quads, within a quad the first-listed triangle first.  A record is 13 bytes, little-endian,
packed: the byte 3, then three int32 vertex indices -- PLY's `property list uchar int vertex_indices`.  Counts: one uint32 per image,
the number of faces.  A plane with h = 1 or w = 1 has no quad: zero faces, accepted."""
import functools

import numpy as np

from tests import cloud_ref as Q
from tests.clean_ref import linked, rel_q16

RUN = 1024                                  # MS_RUN of codon_amd/csrc/mesh_tile.h: consecutive quads per workgroup
REC = 13
RECORD = np.dtype([("n", "u1"), ("v", "<i4", (3,))])
assert RECORD.itemsize == REC
DEFAULTS = dict(tolerance=2, tolerance_rel=0.02)
A_, B_, C_, D_ = 0, 1, 2, 3


def vertex_index(c):
    """(h, w) int64: the rank of a non-zero code among the non-zero codes in row-major order, -1 for a hole"""
    v = np.asarray(c) != 0
    return np.where(v, np.cumsum(v.ravel()).reshape(v.shape) - 1, -1)


def quad_faces(c, tolerance=2, tolerance_rel_q16=1311):
    """(corners (Q, 2, 3) of A_ .. D_, emitted (Q, 2) bool, kind (Q) int) of one (h, w) plane's Q = (h - 1)(w - 1) quads in
    row-major order.  kind: 4 diagonal a-d without a tie, 5 a tie (a-d), 6 diagonal b-c, 0 .. 3 exactly three corners with corner
    kind missing, -1 fewer than three"""
    k = np.asarray(c)
    k = (k.view(np.uint16) if k.dtype == np.int16 else k).astype(np.int64)
    A, Rq = int(tolerance), int(tolerance_rel_q16)
    kc = np.stack([k[:-1, :-1], k[:-1, 1:], k[1:, :-1], k[1:, 1:]], axis=-1).reshape(-1, 4)      # a b c d
    n = len(kc)
    valid = kc != 0
    cnt = valid.sum(axis=1)
    tri = np.zeros((n, 2, 3), dtype=np.int64)
    cand = np.zeros((n, 2), dtype=bool)
    kind = np.full(n, -1, dtype=np.int64)
    four = cnt == 4
    da, db = np.abs(kc[:, A_] - kc[:, D_]), np.abs(kc[:, B_] - kc[:, C_])
    ad, bc = four & (da <= db), four & (da > db)
    tri[ad] = [[A_, C_, D_], [A_, D_, B_]]
    tri[bc] = [[A_, C_, B_], [B_, C_, D_]]
    cand[four] = True
    kind[ad & (da < db)], kind[ad & (da == db)], kind[bc] = 4, 5, 6
    for missing, t in ((D_, [A_, C_, B_]), (A_, [B_, C_, D_]), (B_, [A_, C_, D_]), (C_, [A_, D_, B_])):
        m = (cnt == 3) & ~valid[:, missing]
        tri[m, 0] = t
        cand[m, 0] = True
        kind[m] = missing
    rows = np.arange(n)[:, None]
    ok = cand.copy()
    for x, y in ((0, 1), (1, 2), (0, 2)):
        ok &= linked(kc[rows, tri[:, :, x]], kc[rows, tri[:, :, y]], A, Rq)
    return tri, ok, kind


def faces_plane(c, tolerance=2, tolerance_rel_q16=1311):
    """(F, 3) int32 vertex indices of one (h, w) plane, in the order of the definition"""
    c = np.asarray(c)
    h, w = c.shape
    if h < 2 or w < 2:
        return np.zeros((0, 3), dtype=np.int32)
    tri, ok, _ = quad_faces(c, tolerance, tolerance_rel_q16)
    idx = vertex_index(c)
    corner = np.stack([idx[:-1, :-1], idx[:-1, 1:], idx[1:, :-1], idx[1:, 1:]], axis=-1).reshape(-1, 4)
    v = corner[np.arange(len(corner))[:, None, None], tri]            # (Q, 2, 3)
    out = v[ok]                                                        # row-major over (Q, 2): quads in order, the first triangle first
    assert (out >= 0).all()
    return out.astype(np.int32)


def records(faces):
    """(F, 3) int32 -> the packed 13-byte records"""
    r = np.zeros(len(faces), dtype=RECORD)
    r["n"] = 3
    r["v"] = faces
    return r.tobytes()


def mesh(c, tolerance=2, tolerance_rel_q16=1311):
    """(B, h, w) codes -> ([the face bytes of every image], counts (B) uint32)"""
    f = [faces_plane(p, tolerance, tolerance_rel_q16) for p in np.asarray(c)]
    return [records(x) for x in f], np.array([len(x) for x in f], dtype=np.uint32)


def row_bytes(h, w):
    """the bytes of one image's row of the face buffer"""
    return 2 * (h - 1) * (w - 1) * REC


# ---- the shared cases of the GPU test and of the host-side check ----------------------------------------------------------------------

# (B, h, w): no quad (three ways); one quad; small; exactly one run of RUN quads; a second run that holds one quad; a batch, for the
# per-image offsets; rows that are not aligned; 259 runs, so a scan thread takes more than one word
_SIDE = int(round(RUN ** 0.5))
assert _SIDE * _SIDE == RUN and (RUN + 1) % 25 == 0
SHAPES = ((1, 1, 1), (1, 1, 37), (1, 37, 1), (1, 2, 2), (1, 5, 7), (1, _SIDE + 1, _SIDE + 1), (1, 26, (RUN + 1) // 25 + 1), (3, 9, 33),
          (1, 93, 116), (1, 520, 512))
PATTERNS = Q.PATTERNS + ("holes", "saddle")
TOLERANCES = ("zero", "default", "top")
BIG = SHAPES[9]
BIG_CASES = (("random", "default"), ("all", "top"), ("holes", "default"), ("saddle", "zero"))     # of the 520 x 512 plane
SADDLE_DELTA = 2                            # inside the default tolerance


def top_of(pattern):
    return Q.top_of(pattern) if pattern in Q.PATTERNS else 10000


def tolerance_of(name, top):
    return {"zero": 0, "default": DEFAULTS["tolerance"], "top": top}[name]


RQ = rel_q16(DEFAULTS["tolerance_rel"])


@functools.lru_cache(maxsize=None)
def plane(shape, pattern):
    """(B, h, w) codes of a pattern, read-only: cloud_ref's, and
    holes   a smooth surface with isolated single pixels three apart, by turns a hole -- it is each of the four corners of a quad
            of three -- and a flying pixel far from everything, whose four quads emit exactly one triangle
    saddle  base + ((i + j) % 2) delta with a slow ramp over it: both diagonals, and ties where the ramp is flat"""
    if pattern in Q.PATTERNS:
        return Q.plane(shape, pattern)
    B, h, w = shape
    top = top_of(pattern)
    i, j = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    if pattern == "holes":
        c = np.broadcast_to(top // 2 + i + j, shape).astype(np.int64).copy()
        at = (i % 3 == 1) & (j % 3 == 1)                              # 3 apart: no quad holds two
        c[:, at & ((i // 3 + j // 3) % 2 == 0)] = 0
        c[:, at & ((i // 3 + j // 3) % 2 == 1)] = top                 # a flying pixel: linked to nothing below the tolerance `top`
    else:
        assert pattern == "saddle"
        c = np.broadcast_to(top // 2 + ((i + j) % 2) * SADDLE_DELTA + (j // 3) % 3 - (i // 4) % 2, shape).astype(np.int64)
    out = c.astype(np.uint16)
    out.setflags(write=False)
    return out


def cases(shape):
    """[(pattern, tolerance name)] of a shape: every pattern under every tolerance, but the 520 x 512 plane under BIG_CASES alone"""
    if tuple(shape) == BIG:
        return list(BIG_CASES)
    return [(pattern, tol) for pattern in PATTERNS for tol in TOLERANCES]


@functools.lru_cache(maxsize=None)
def want(shape, pattern, tol):
    """(face bytes per image [bytes], counts (B) uint32) of a case, computed once"""
    bodies, counts = mesh(plane(shape, pattern), tolerance_of(tol, top_of(pattern)), RQ)
    counts.setflags(write=False)
    return tuple(bodies), counts


# codon_cloud_mesh's refusals: (what differs from a good call of u16 codes on a 5 x 7 plane, a piece of the message)
REFUSALS = [({"src": None}, "null pointer"), ({"faces": None}, "null pointer"), ({"counts": None}, "null pointer"),
            ({"ws": None}, "null pointer"),
            ({"fmt": 2}, "fmt 2 "), ({"fmt": -1}, "fmt -1 "), ({"B": 0}, "batch 0 "), ({"B": 65536}, "batch 65536 "),
            ({"h": 0}, "a 0x7 plane"), ({"w": 0}, "a 5x0 plane"), ({"h": 4097}, "a 4097x7 plane"), ({"w": 4097}, "a 5x4097 plane"),
            ({"top": 0}, "top 0 "), ({"top": 65536}, "top 65536 "), ({"fmt": 0, "top": 1000}, "top 1000 "),
            ({"tol_abs": -1}, "tolerance -1 "), ({"top": 10000, "tol_abs": 10001}, "tolerance 10001 "),
            ({"tol_rel": -1}, "tolerance_rel -1 "), ({"tol_rel": 65536}, "tolerance_rel 65536 "),
            ({"ws_bytes": "short"}, "too small")]
