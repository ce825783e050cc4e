"""tests/bounds.py checks itself: round16 against single-rounded conversions known to be correct, and assert_rounded
accepts a correctly rounded conv and rejects the wrong ones a whole-tensor RMSE bar lets through (a truncating store, one
element 2 ulps off, one element never written, a tau so wide that the check decides nothing).  CPU only."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from codon_amd import _lib as L
from tests.bounds import assert_rounded, conv_ref, round16, tau_of, ulp

DT16 = [torch.bfloat16, torch.float16]


def _rand(shape, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(size=shape) * scale).astype(np.float32))


def _edge_values(seed):
    """float64 values around every region of both 16-bit formats: random magnitudes over the whole range, values on
    and next to the ties of bf16 and fp16, subnormals of both, and both formats' overflow thresholds."""
    g = np.random.default_rng(seed)
    mag = np.ldexp(g.uniform(1, 2, 20000), g.integers(-150, 130, 20000))
    v = [mag * g.choice([-1.0, 1.0], mag.size)]
    for bits, emin in [(8, -133), (11, -24)]:
        e = g.integers(emin + bits - 1, 16, 4000)
        m = g.integers(2 ** (bits - 1), 2 ** bits, e.size).astype(np.float64)
        tie = np.ldexp(m + 0.5, e - bits)                        # halfway between two numbers of the format
        v += [tie, -tie, np.nextafter(tie, np.inf), np.nextafter(tie, -np.inf)]
        sub = np.ldexp(g.integers(0, 2 ** (bits - 1), 2000).astype(np.float64) + g.choice([0.0, 0.5, 0.25], 2000), emin)
        v += [sub, -sub]
    v += [np.array([65504.0, 65519.99, 65520.0, 65536.0, 1e300, -1e300, 0.0, -0.0, 3.3895313892515355e38,
                    3.3961775292304e38, 2.0 ** 128 * (1 - 2.0 ** -9), 2.0 ** 128 * (1 - 2.0 ** -9.5)])]
    return np.concatenate(v)


def test_round16_fp16_matches_single_rounded_cast():
    x = _edge_values(1)
    with np.errstate(over="ignore"):
        ref = x.astype(np.float16).astype(np.float64)
    got = round16(x, torch.float16)
    assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    assert round16([2.0 ** -25], torch.float16)[0] == 0.0 and round16([2.0 ** -25 * 1.5], torch.float16)[0] == 2.0 ** -24
    assert round16([65520.0], torch.float16)[0] == np.inf and round16([65519.99], torch.float16)[0] == 65504.0


def test_round16_bf16_matches_torch_on_fp32_values():
    """On values that are exact fp32 numbers torch's fp32 -> bf16 cast is a single rounding (ties to even, subnormals,
    overflow to inf): round16 must agree with it bit for bit."""
    x = _edge_values(2)
    with np.errstate(over="ignore"):
        x32 = x.astype(np.float32)
    x32 = x32[np.isfinite(x32)]
    ref = torch.from_numpy(x32).to(torch.bfloat16).double().numpy()
    got = round16(x32.astype(np.float64), torch.bfloat16)
    assert np.array_equal(got, ref) and np.array_equal(np.signbit(got), np.signbit(ref))
    big = np.float32(3.3961775e38)                                   # just past bf16's max finite + half ulp
    assert round16([float(big)], torch.bfloat16)[0] == float(torch.tensor(big).to(torch.bfloat16).double())
    assert round16([2.0 ** 128 * (1 - 2.0 ** -9)], torch.bfloat16)[0] == np.inf          # the tie above the max: to even
    assert round16([2.0 ** 128 * (1 - 2.0 ** -8)], torch.bfloat16)[0] == 2.0 ** 128 * (1 - 2.0 ** -8)
    assert round16([2.0 ** -134], torch.bfloat16)[0] == 0.0 and round16([2.0 ** -134 * 1.5], torch.bfloat16)[0] == 2.0 ** -133


@pytest.mark.parametrize("dtype", DT16)
def test_round16_rounds_once_from_float64(dtype):
    """1 + half an ulp + 2^-30 lies just above a tie: one rounding goes up.  torch's float64 -> 16-bit .to() first rounds
    to float32, lands ON the tie and goes to even (down) -- the double rounding round16 exists to avoid."""
    half = 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -11
    x = np.array([1 + half + 2.0 ** -30, -(1 + half + 2.0 ** -30), 1 + half, 1 + 3 * half, 1 + 3 * half - 2.0 ** -40])
    assert list(round16(x, dtype)) == [1 + 2 * half, -(1 + 2 * half), 1.0, 1 + 4 * half, 1 + 2 * half]
    assert float(torch.tensor(x[0], dtype=torch.float64).to(dtype).double()) == 1.0     # what the torch cast gives
    assert round16(np.array([np.nan]), dtype)[0] != round16(np.array([np.nan]), dtype)[0]


def test_ulp():
    assert ulp([1.0], torch.bfloat16)[0] == 2.0 ** -7 and ulp([1.0], torch.float16)[0] == 2.0 ** -10
    assert ulp([1.5], torch.float32)[0] == 2.0 ** -23 and ulp([0.0], torch.float16)[0] == 2.0 ** -24


def _sim_case(dtype, k=3, cin=64, cout=64, shape=(2, 19, 45), pack=L.PACK_FWD, seed=0):
    """The GPU tests' data recipe: standard-normal x, weights scaled by (2 / (k^2 cout))^1/2, both rounded to dtype."""
    B, H, W = shape
    q = (lambda t: t.to(dtype).float()) if dtype != torch.float32 else (lambda t: t)
    cx, cw = (cout, (cout, cin)) if pack == L.PACK_DGRAD else (cin, (cout, cin))
    x = q(_rand((B, cx, H, W), seed + 1))
    w = q(_rand((*cw, k, k), seed + 2, scale=(2.0 / (k * k * cout)) ** 0.5))
    return x, w


def _store(v64, dtype):
    return torch.from_numpy(round16(v64.numpy(), dtype)) if dtype != torch.float32 else v64.float().double()


def test_conv_ref_forward_and_dgrad():
    """conv_ref states the conv the kernel computes: PACK_FWD is conv2d, PACK_DGRAD the input gradient of that conv."""
    x, w = _sim_case(torch.float32, k=5, cin=64, cout=128, shape=(1, 7, 9))
    ref, S = conv_ref(x, w, 5, L.PACK_FWD)
    assert ref.dtype == torch.float64 and torch.allclose(ref, F.conv2d(x.double(), w.double(), None, 1, 2))
    assert (S >= ref.abs()).all() and torch.allclose(S, F.conv2d(x.double().abs(), w.double().abs(), None, 1, 2))
    gy = _rand((1, 128, 7, 9), 3)
    xr = x.double().requires_grad_(True)
    F.conv2d(xr, w.double(), None, 1, 2).backward(gy.double())
    gx, _ = conv_ref(gy, w, 5, L.PACK_DGRAD)
    assert gx.shape == x.shape and torch.allclose(gx, xr.grad, rtol=0, atol=1e-12)


@pytest.mark.parametrize("dtype", DT16 + [torch.float32])
def test_accepts_correctly_rounded_conv(dtype):
    x, w = _sim_case(dtype)
    ref, S = conv_ref(x, w, 3)
    r = _rand(ref.shape, 9)
    r = r.to(dtype).double() if dtype != torch.float32 else r.double()
    s = assert_rounded(_store(ref, dtype), ref, tau_of(S), dtype, f"sim plain {dtype}", S=S)
    assert s["max_err_over_S"] < (0.02 if dtype == torch.bfloat16 else 3e-3 if dtype == torch.float16 else 1e-7)
    if dtype != torch.float32:                   # tau ~ 5e-5 |ref| against half-ulps of 2-4e-3 (bf16), 2.4-4.9e-4 (fp16)
        assert s["exact_share"] > (0.97 if dtype == torch.bfloat16 else 0.8)
    assert_rounded(_store(torch.relu(ref), dtype), ref, tau_of(S), dtype, "sim relu", epi=torch.relu, S=S)
    assert_rounded(_store(ref + r, dtype), ref, tau_of(S, r), dtype, "sim residual", epi=lambda a: a + r, S=S)
    # an accumulator error of 8 fp32 units of S (half of tau), before the rounding, still passes
    a = ref + 2.0 ** -21 * S * torch.from_numpy(np.random.default_rng(4).uniform(-1, 1, ref.shape))
    assert_rounded(_store(a, dtype), ref, tau_of(S), dtype, "sim perturbed", S=S)


@pytest.mark.parametrize("dtype", DT16)
def test_rejects_truncating_store(dtype):
    x, w = _sim_case(dtype)
    ref, S = conv_ref(x, w, 3)
    r = round16(ref.numpy(), dtype)
    # toward zero: where rounding went away from zero, step back one spacing (at a power of two, the finer one below)
    below = np.abs(r) - ulp(np.nextafter(np.abs(r), 0), dtype)
    trunc = np.where(np.abs(r) > np.abs(ref.numpy()), np.sign(r) * below, r)
    assert np.all(np.abs(trunc) <= np.abs(ref.numpy())) and (trunc != r).mean() > 0.3
    with pytest.raises(AssertionError, match="elements outside the correctly rounded interval"):
        assert_rounded(torch.from_numpy(trunc), ref, tau_of(S), dtype, "sim truncated")


@pytest.mark.parametrize("dtype", DT16)
def test_rejects_one_element_two_ulps_off_and_names_it(dtype):
    x, w = _sim_case(dtype, k=5, cin=128, cout=128, shape=(1, 33, 70))
    ref, S = conv_ref(x, w, 5)
    got = torch.from_numpy(round16(ref.numpy(), dtype))
    b, c, h, wi = 0, 77, 31, 65
    v = float(got[b, c, h, wi])
    got[b, c, h, wi] = v + 2 * float(ulp([v], dtype)[0])
    with pytest.raises(AssertionError) as e:
        assert_rounded(got, ref, tau_of(S), dtype, "sim 2 ulp")
    assert "1 of " in str(e.value) and f"(b,c,h,w)=({b}, {c}, {h}, {wi})" in str(e.value), str(e.value)


@pytest.mark.parametrize("dtype", DT16 + [torch.float32])
def test_rejects_one_nan(dtype):
    x, w = _sim_case(dtype)
    ref, S = conv_ref(x, w, 3)
    got = _store(ref, dtype)
    got[1, 5, 18, 44] = float("nan")
    with pytest.raises(AssertionError, match=r"(?s)1 of .*\(b,c,h,w\)=\(1, 5, 18, 44\): got nan"):
        assert_rounded(got, ref, tau_of(S), dtype, "sim nan")


@pytest.mark.parametrize("dtype", DT16)
def test_rejects_an_uninformative_tau(dtype):
    """A tau of 2^-8 S lets most elements take two or more values: the check must fail instead of passing."""
    x, w = _sim_case(dtype)
    ref, S = conv_ref(x, w, 3)
    got = torch.from_numpy(round16(ref.numpy(), dtype))
    assert_rounded(got, ref, 2.0 ** -18 * S, dtype, "sim tau 2^-18 S")          # the widest tau the issue allows
    with pytest.raises(AssertionError, match="single allowed value"):
        assert_rounded(got, ref, 2.0 ** -8 * S, dtype, "sim tau 2^-8 S")
