"""The cases the GPU test of the temporal stream (tests/test_gpu_temporal_stream.py) and its host-side check
(tools/host_check.py temporal_push) share -- TEST INFRASTRUCTURE.  A case is a row of tests/temporal_ref.py's form,
(T, h, w, Bk, Ah, M, F, A, Rq, pattern, top), so temporal_ref.sequence and temporal_ref.want serve it: the expectation of a stream
is the restatement of the WHOLE sequence.

Planes: temporal_ref.PLANES -- one pixel, a single row, a partial last quad at 9 x 29, whole quads at 4 x 8, four pixel groups with a
partial last one at 40 x 100.  Windows: all seven of temporal_ref.WINDOWS, so every count of window registers is taken.  Lengths:
1, 2, ahead, ahead + 1, 15, 16, 17 and 33 -- at T <= ahead every output comes from the flush, 16 fills the ring, 17 wraps it, 33
wraps it twice; the large plane runs 1, 3 and 17 alone.  Parameters, patterns and formats in turn, by the index arithmetic of
temporal_ref.cases."""
from tests import temporal_ref as R

BIG_LENGTHS = (1, 3, 17)


def lengths(plane, window):
    """The T of a plane under a window, ascending; duplicates and zeros dropped"""
    if plane == R.BIG_PLANE:
        return BIG_LENGTHS
    ahead = window[1]
    return tuple(sorted({1, 2, ahead, ahead + 1, 15, 16, 17, 33} - {0}))


def cases():
    """[(T, h, w, Bk, Ah, M, F, A, Rq, pattern, top)]: every plane under every window at every length"""
    rows = []
    for pi, plane in enumerate(R.PLANES):
        for wi, window in enumerate(R.WINDOWS):
            for ti, T in enumerate(lengths(plane, window)):
                M, F, A, Rq = R.PARAMS[(pi + wi + ti) % len(R.PARAMS)]
                pattern = R.PATTERNS[(pi + 2 * wi + 3 * ti) % len(R.PATTERNS)]
                top = 65535 if pattern == "high" else R.FORMATS[(pi + wi + 2 * ti) % 3][1]
                rows.append((T, *plane, *window, M, F, R.SCENE_TOLERANCE[top] if A is None else A,
                             R.rel_q16(R.DEFAULTS["tolerance_rel"]) if Rq is None else Rq, pattern, top))
    return rows


def emitted_by(T, ahead):
    """[(frame, step)] of a stream of T frames: frame t is the answer of push t + ahead (step t + ahead), or of flush step
    t - max(0, T - ahead) (step T + that) -- T outputs for T inputs, in order"""
    first = max(0, T - ahead)
    return [(t, t + ahead if t < first else T + t - first) for t in range(T)]
