"""tests/bounds.py checks itself: round16 against single-rounded conversions known to be correct, and assert_rounded
accepts a correctly rounded conv and rejects the wrong ones a whole-tensor RMSE bar lets through (a truncating store, one
element 2 ulps off, one element never written, a tau so wide that the check decides nothing).  The weight-gradient helpers:
the restated band planner equals the library's, the probe pixels cover the seams, the one-hot expectation equals float64
conv2d_weight, and assert_wgrad passes torch's fp32 result, fails ONE removed product at the largest K, refuses K over its cap.
CPU only."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from codon_amd import _lib as L
from tests.bounds import (WGRAD_K_CAP, assert_rounded, assert_wgrad, conv_ref, round16, tau_of, ulp, wgrad_bands,
                          wgrad_impulse_diff, wgrad_impulse_expect, wgrad_one_hot, wgrad_probe_pixels, wgrad_ref)

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


# ---- weight gradients -------------------------------------------------------------------------------------------------

WGRAD_FORMS = [(5, 128, 128), (5, 64, 64), (3, 64, 64), (3, 128, 64), (1, 128, 64)]


def test_wgrad_bands_restates_the_library_planners():
    """nsplit of wgrad_bands == codon_conv_wgrad_workspace_bytes / (4 cout cin k^2) (a host function: no GPU) over a grid of
    batches and image sizes, 16-bit and fp32, W % 4 == 0 and not; the bands tile the tile rows."""
    lib = L.load()
    for dtype, code in ((torch.bfloat16, L.BF16), (torch.float16, L.F16), (torch.float32, L.F32)):
        for k, cin, cout in WGRAD_FORMS:
            for B in (1, 2, 3, 7, 11, 16, 32, 65, 128, 257, 512):
                for H in (1, 3, 9, 20, 41, 44, 61, 128, 130, 480):
                    for W in (33, 40, 63, 640):
                        d = L.ConvDesc(B, H, W, cin, cout, k, cin + 64, 64, cout + 64, 64, 0, 0, 0, code)
                        n = lib.codon_conv_wgrad_workspace_bytes(C.byref(d)) // (4 * cout * cin * k * k)
                        for aligned in (True, False):
                            p = wgrad_bands(dtype, k, cin, cout, B, H, W, aligned=aligned)
                            assert p["nsplit"] == n, (dtype, k, cin, cout, B, H, W, n, p)
                            assert sum(p["rows_per_band"]) == p["tiles"] == -(-H // p["th"]) and min(p["rows_per_band"]) >= 1
    # the plans the issue names: the CLI default and bench.py --mode train, 5x5 128 -> 128 in bf16
    assert wgrad_bands(torch.bfloat16, 5, 128, 128, 16, 128, 128)["rows_per_band"] == [6, 7]
    assert wgrad_bands(torch.bfloat16, 5, 128, 128, 32, 480, 640)["rows_per_band"] == [48]
    assert wgrad_bands(torch.bfloat16, 1, 128, 64, 32, 480, 640)["rows_per_band"] == [15] * 8
    assert wgrad_bands(torch.bfloat16, 5, 64, 64, 1, 130, 40)["rows_per_band"] == [1] * 13       # test_conv2d_wgrad_slices_and_bands


@pytest.mark.parametrize("dtype,k,shape,aligned", [(torch.bfloat16, 5, (16, 128, 128), True), (torch.bfloat16, 3, (65, 49, 33), True),
                                                   (torch.float32, 1, (20, 53, 40), True), (torch.float32, 5, (11, 25, 40), False),
                                                   (torch.float16, 1, (3, 7, 63), True)])
def test_wgrad_probe_pixels_cover_the_seams(dtype, k, shape, aligned):
    B, H, W = shape
    cin, cout = (128, 128) if k == 5 else (64, 64) if k == 3 else (128, 64)
    plan = wgrad_bands(dtype, k, cin, cout, B, H, W, aligned=aligned)
    rounds = wgrad_probe_pixels(plan, B, H, W, cout)
    assert all(len(r) == cout for r in rounds)
    pix = [p for r in rounds for p in r]
    assert all(0 <= b < B and 0 <= h < H and 0 <= w < W for b, h, w in pix)
    rows, cols, imgs = {h for _, h, _ in pix}, {w for _, _, w in pix}, {b for b, _, _ in pix}
    for t in range(1, plan["tiles"]):                                     # both sides of every tile-row seam, band seams included
        assert t * plan["th"] - 1 in rows and t * plan["th"] in rows, (t, sorted(rows))
    assert {0, H - 1} <= rows and {0, W - 1, (W - 1) // 32 * 32} <= cols and {0, B // 2, B - 1} <= imgs
    if W > 32:
        assert {31, 32} <= cols
    assert {(h, w) for _, h, w in pix} >= {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1)}


@pytest.mark.parametrize("k", [1, 3, 5])
def test_wgrad_impulse_expect_equals_float64_conv2d_weight(k):
    B, H, W, cin, cout = 3, 9, 37, 8, 16
    plan = wgrad_bands(torch.float32, k, 128, 64, B, H, W)
    x, gy = _rand((B, cin, H, W), 1).double(), _rand((B, cout, H, W), 2).double()
    pix = wgrad_probe_pixels(plan, B, H, W, cout)[0]
    hot = wgrad_one_hot(pix, B, H, W).double()
    ref, _ = wgrad_ref(x, hot, k)
    assert torch.equal(wgrad_impulse_expect(x, pix, k, "gy"), ref)
    pix = pix[:cin]
    hot = wgrad_one_hot(pix, B, H, W).double()
    ref, _ = wgrad_ref(hot, gy, k)
    exp = wgrad_impulse_expect(gy, pix, k, "x")
    assert exp.shape == ref.shape and torch.equal(exp, ref)
    assert wgrad_impulse_diff(ref, exp, pix, k, "x", plan) is None


def test_wgrad_impulse_diff_names_the_seam():
    """A band that drops the first halo row of its second tile row: the message names the element, the pixel, its band and
    tile row, and that the product is missing."""
    k, B, H, W = 5, 16, 128, 128
    plan = wgrad_bands(torch.bfloat16, 5, 128, 128, B, H, W)
    x = _rand((B, 4, H, W), 3)
    pix = wgrad_probe_pixels(plan, B, H, W, 128)[0]
    exp = wgrad_impulse_expect(x, pix, k, "gy")
    co = next(i for i, (_, h, _) in enumerate(pix) if h == 70)           # first row of tile row 7 = the first of band 1
    b, h, w = pix[co]
    got = exp.clone()
    got[co, :, 0, :] = 0                                                  # x row h - 2: the first halo row
    msg = wgrad_impulse_diff(got, exp, pix, k, "gy", plan)
    assert f"(co,ci)=({co}, 0) tap (dy,dx)=(0, " in msg and "product missing" in msg, msg
    assert f"gy pixel (b,h,w)=({b}, 70, {w})" in msg and "band 1 of 2 (tile rows 6..12), tile row 7 (rows 70..79)" in msg, msg
    got = exp.clone()
    got[co] *= 2
    assert "product counted twice" in wgrad_impulse_diff(got, exp, pix, k, "gy", plan)
    got = exp.clone()
    got[co, :, 1, 1] = exp[co, :, 1, 2]
    assert "the value expected at tap (1, 2)" in wgrad_impulse_diff(got, exp, pix, k, "gy", plan)


@pytest.mark.parametrize("dtype", DT16 + [torch.float32])
def test_assert_wgrad_passes_torch_fp32(dtype):
    B, H, W, k = 32, 44, 40, 5
    q = (lambda t: t.to(dtype).float()) if dtype != torch.float32 else (lambda t: t)
    x, gy = q(_rand((B, 16, H, W), 1)), q(_rand((B, 8, H, W), 2))
    ref, S = wgrad_ref(x, gy, k)
    assert ref.dtype == torch.float64 and tuple(ref.shape) == (8, 16, 5, 5) and (S >= ref.abs()).all()
    got = torch.nn.grad.conv2d_weight(x, (8, 16, k, k), gy, padding=2)
    s = assert_wgrad(got, ref, S, f"torch fp32 {dtype}", K=B * H * W)
    assert s["max_err_over_S"] < 2.0 ** -22                              # fp32 summation: a few units of 2^-24 S
    bad = got.clone()
    bad[3, 5, 2, 2] = float("nan")
    with pytest.raises(AssertionError, match=r"(?s)1 of .*\(co,ci,dy,dx\)=\(3, 5, 2, 2\): got nan"):
        assert_wgrad(bad, ref, S, "sim nan", K=B * H * W)


def test_assert_wgrad_fails_one_removed_product_at_the_largest_K():
    """K = 16 x 128 x 128 = 2^18, exactly on the cap (the largest GPU case): the float64 reference with ONE product of
    median size taken out of one element must fail, and the message must name the element."""
    B, H, W, k, cin, cout = 16, 128, 128, 5, 4, 4
    assert B * H * W == WGRAD_K_CAP
    x, gy = _rand((B, cin, H, W), 1).bfloat16().float(), _rand((B, cout, H, W), 2).bfloat16().float()
    ref, S = wgrad_ref(x, gy, k)
    assert_wgrad(ref.float(), ref, S, "sim fp32-rounded reference", K=B * H * W)
    for co, ci, dy, dx in [(0, 0, 0, 0), (3, 1, 2, 2), (1, 3, 4, 1)]:
        xs = F.pad(x[:, ci].double(), (2, 2, 2, 2))[:, dy:dy + H, dx:dx + W]
        prod = (gy[:, co].double() * xs).flatten()
        assert abs(float(prod.sum()) - float(ref[co, ci, dy, dx])) < 1e-9
        med = prod.abs().median()
        i = int((prod.abs() - med).abs().argmin())
        for scale in (-1.0, 1.0):                                        # the product dropped; the product counted twice
            got = ref.clone()
            got[co, ci, dy, dx] += scale * prod[i]
            with pytest.raises(AssertionError, match=rf"(?s)1 of .*\(co,ci,dy,dx\)=\({co}, {ci}, {dy}, {dx}\)"):
                assert_wgrad(got, ref, S, "sim one product", K=B * H * W)


def test_assert_wgrad_refuses_a_case_over_the_K_cap():
    ref = torch.ones((2, 2, 1, 1), dtype=torch.float64)
    assert_wgrad(ref, ref, ref, "sim on the cap", K=WGRAD_K_CAP)
    with pytest.raises(AssertionError, match="cannot see one dropped product"):
        assert_wgrad(ref, ref, ref, "sim over the cap", K=WGRAD_K_CAP + 1)


def test_wgrad_cases_cover_every_plan_class_per_form_and_dtype():
    """The case table itself: per kernel family, dtype and form one band of >= 3 tile rows, uneven bands, and nsplit below 8,
    a multiple of 8 and 8 n + r; W % 32 takes 1, 8 and 31 (8 alone where the kernel needs W % 4 == 0).  The planner is a host
    function, so a planner change that empties a plan class shows here, without a GPU."""
    from tests import test_gpu_wgrad_plans as P
    seen = {}
    for prm in P._cases():
        fam, dtype, form, cls, shape, aligned = prm.values
        plan = wgrad_bands(dtype, *form, *shape, aligned=aligned)
        assert plan["nsplit"] == P._nsplit(dtype, *form, *shape)
        s = seen.setdefault((fam, dtype, form), {"rows3": False, "uneven": False, "ns": set(), "wmod": set()})
        s["rows3"] |= max(plan["rows_per_band"]) >= 3
        s["uneven"] |= len(set(plan["rows_per_band"])) > 1
        s["ns"].add("<8" if plan["nsplit"] < 8 else "8n" if plan["nsplit"] % 8 == 0 else "8n+r")
        s["wmod"].add(shape[2] % 32)
    assert len(seen) == 4 * len(P.FORMS)
    for key, s in seen.items():
        assert s["rows3"] and s["uneven"] and s["ns"] == {"<8", "8n", "8n+r"}, (key, s)
    for fam, want in (("c8", {1, 8, 31}), ("f32_t16", {8}), ("f32_r1", {1, 31, 8})):
        got = set().union(*(s["wmod"] for (f, _, _), s in seen.items() if f == fam))
        assert want <= got, (fam, got)


def test_wgrad_impulse_diff_calls_a_pixel_past_the_ragged_edge_outside():
    """One-hot x on the last row: the taps whose gy pixel lies below the image (rows H .. tiles th - 1 of the ragged last
    tile row) or right of it are 'outside the image', not given a band."""
    k, B, H, W = 5, 3, 19, 33
    plan = wgrad_bands(torch.bfloat16, 5, 128, 128, B, H, W)
    assert plan["tiles"] * plan["th"] > H
    gy = _rand((B, 4, H, W), 5)
    pix = [(1, H - 1, W - 1)]
    exp = wgrad_impulse_expect(gy, pix, k, "x")
    got = exp.clone()
    got[0, 0, 0, 4] = 1.0                                                 # gy pixel (H + 1, W - 3): below the image
    got[0, 0, 4, 0] = 2.0                                                 # gy pixel (H - 3, W + 1): right of it
    got[0, 0, 2, 2] += 1.0                                                # gy pixel (H - 1, W - 1): the last tile row
    lines = wgrad_impulse_diff(got, exp, pix, k, "x", plan).splitlines()
    assert len(lines) == 4 and lines[1].endswith("outside the image") and lines[3].endswith("outside the image"), lines
    assert f"tile row {plan['tiles'] - 1} " in lines[2] and "tile column 1" in lines[2], lines
