"""Pins tests/d4_ref.py, the numpy definition of the D4 self-ensemble that the kernels of csrc/d4.hip are held
to on the GPU (tests/test_gpu_d4.py): its views are the training augmentation's D4 op, inverse-of-view is the identity, the
two view batches are laid out as the C ABI states, and the merge's tree order makes eight equal values average to themselves
exactly -- where a running sum would not."""
import ctypes as C

import numpy as np
import pytest

from tests import d4_ref as D
from tests import train_data_ref as R


def test_views_are_the_training_augmentation():
    g = np.random.default_rng(0)
    c = g.integers(0, 256, size=(9, 9)).astype(np.uint8)
    for op in range(8):
        assert np.array_equal(D.view(c, op), R.d4(c, op)), op
    assert len({D.view(c, op).tobytes() for op in range(8)}) == 8          # eight different views


def test_inverse_of_view_is_the_identity_on_a_non_square_plane():
    c = np.arange(5 * 7, dtype=np.float32).reshape(5, 7)
    for op in range(8):
        v = D.view(c, op)
        assert v.shape == ((7, 5) if op & 1 else (5, 7)), op
        assert np.array_equal(D.inverse(v, op), c), op
    assert D.UPRIGHT == (0, 2, 4, 6) and D.TRANSPOSED == (1, 3, 5, 7)


def test_view_batches_layout():
    x = np.arange(3 * 5 * 7, dtype=np.float32).reshape(3, 1, 5, 7)
    up, tr = D.views(x)
    assert up.shape == (12, 1, 5, 7) and tr.shape == (12, 1, 7, 5)
    for b in range(3):
        for k in range(8):
            got = (tr if k & 1 else up)[4 * b + (k >> 1), 0]
            assert np.array_equal(got, D.view(x[b, 0], k)), (b, k)
    # bits are copied: NaN payloads and -0.0 survive, in a 16-bit container too
    bits = np.array([0x7FC1, 0xFFFF, 0x8000, 0x0001, 0x7C00, 0x3C00], dtype=np.uint16).reshape(1, 1, 2, 3)
    ub, tb = D.views(bits)
    assert ub.dtype == tb.dtype == np.uint16 and np.array_equal(ub[0], bits[0]) and np.array_equal(tb[0, 0], bits[0, 0].T)
    assert np.array_equal(np.sort(ub.reshape(4, -1), axis=1), np.sort(tb.reshape(4, -1), axis=1))


def test_merge_of_eight_equal_planes_returns_the_planes_bits():
    g = np.random.default_rng(1)
    # values whose 3*x, 5*x, 6*x, 7*x are inexact in fp32 (full 24-bit significands), tiny and huge ones, both zeros
    x = np.concatenate([g.uniform(-2, 2, size=29).astype(np.float32),
                        np.array([1e-3, 1.0 + 2.0 ** -23, 3.4e38 / 16, 1e-45, -0.0, 0.0], dtype=np.float32)]).reshape(1, 1, 5, 7)
    up, tr = D.views(x)
    out = D.merge(up, tr)
    assert out.dtype == np.float32 and np.array_equal(out.view(np.uint32), x.view(np.uint32))
    # the tree order matters: a running sum of the same eight values rounds at 3x (and again later) for some of them
    run = np.zeros_like(x)
    for _ in range(8):
        run = run + x
    assert run.dtype == np.float32
    three = (x + x) + x
    assert np.any(three.astype(np.float64) != 3.0 * x.astype(np.float64))      # 3*x does round for these values
    assert np.any((np.float32(0.125) * run).view(np.uint32) != x.view(np.uint32))


def test_merge_undoes_each_view_and_keeps_its_order():
    """A non-equivariant stand-in: the model adds a position ramp sized to its input, so a wrong inverse or a wrong slot
    changes the result; against float64 arithmetic on the same eight planes the fp32 tree is within 4 ulp."""
    g = np.random.default_rng(2)
    x = g.uniform(0, 1, size=(2, 1, 5, 7)).astype(np.float32)

    def model(a, b):
        n, _, h, w = a.shape
        return (a + np.arange(h * w, dtype=np.float32).reshape(1, 1, h, w) / np.float32(64)).astype(np.float32)

    out = D.self_ensemble(model, x, x, "f32")
    want = np.zeros(x.shape, dtype=np.float64)
    for b in range(2):
        for k in range(8):
            v = D.view(x[b, 0], k)
            o = model(v[None, None], None)[0, 0]
            want[b, 0] += D.inverse(o, k).astype(np.float64) / 8
    assert np.max(np.abs(out - want)) <= 4 * np.spacing(np.float32(np.abs(want).max()))
    assert np.abs(out - x).max() > 0.05                                          # the ramp does not cancel


def test_upcast_is_exact():
    h = np.array([1.0, -0.0, 6.1e-5, 5.96e-8, 65504.0], dtype=np.float16)
    assert np.array_equal(D.upcast(h, "f16").astype(np.float16).view(np.uint16), h.view(np.uint16))
    b = np.array([0x3F80, 0x8000, 0x0001, 0x7F7F], dtype=np.uint16)
    assert np.array_equal(D.upcast(b, "bf16").view(np.uint32), b.astype(np.uint32) << 16)
    with pytest.raises(AssertionError):
        D.upcast(h, "f32")


def test_entry_points_refuse_bad_arguments_without_gpu():
    """Validation happens before any HIP call: NULLs, non-positive sizes and an unknown dtype are BAD_ARG with a message."""
    from codon_amd import _lib as L
    lib = L.load()
    p = C.c_void_p(4096)              # never dereferenced: every call below is refused
    assert lib.codon_d4_views(1, 4, 4, None, None, L.F32, p, p, None, None, None) == -1
    assert b"d4_views" in lib.codon_last_error_string()
    assert lib.codon_d4_views(1, 4, 4, p, None, L.F32, None, p, None, None, None) == -1
    assert lib.codon_d4_views(1, 4, 4, p, None, L.F32, p, None, None, None, None) == -1
    assert lib.codon_d4_views(1, 4, 4, p, p, L.F32, p, p, None, p, None) == -1        # src1 without both of its outputs
    assert lib.codon_d4_views(1, 4, 4, p, None, L.F32, p, p, p, None, None) == -1     # an output of src1 without src1
    for shape in ((0, 4, 4), (1, 0, 4), (1, 4, -1)):
        assert lib.codon_d4_views(*shape, p, None, L.F32, p, p, None, None, None) == -1 and b"bad shape" in lib.codon_last_error_string()
        assert lib.codon_d4_merge(*shape, p, p, L.F32, p, None) == -1 and b"bad shape" in lib.codon_last_error_string()
    assert lib.codon_d4_views(1, 4, 4, p, None, 3, p, p, None, None, None) == -1 and b"dtype" in lib.codon_last_error_string()
    assert lib.codon_d4_merge(1, 4, 4, p, p, -1, p, None) == -1 and b"dtype" in lib.codon_last_error_string()
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.codon_d4_merge(1, 4, 4, args[0], args[1], L.F16, args[2], None) == -1
        assert b"d4_merge: null pointer" in lib.codon_last_error_string()
