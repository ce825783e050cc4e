"""The weight-gradient kernels on the band plans a training run uses: several tile rows per band, uneven bands, ragged last
tiles, and every shape of the fixed-order reduce's loop -- element by element.

Every conv weight gradient comes from conv_wgrad_c8.hip (bf16 / fp16), conv_wgrad_f32_t16.hip (fp32, W % 4 == 0 and 16-byte
aligned slices) or conv_wgrad_f32.hip (fp32 otherwise; also wgrad_reduce_kernel).  A launch cuts every image into nbands
bands of tile rows; want = ceil(target / (channel blocks x B)), clipped to the tile rows.  At B <= 3 on small images want
exceeds the tile rows: every band is ONE tile row, which is all test_gpu_kernels.py and test_gpu_c8.py reach.  Batch drives
the plan, so the cases here get training's plans from large B on small images.

The plan is a stated premise: nsplit = codon_conv_wgrad_workspace_bytes / (4 cout cin k^2) must equal the restated planner
(tests/bounds.py: wgrad_bands), and every case asserts its plan class on it before it launches:
  one_band  nbands == 1 over >= 3 tile rows (nsplit = B, a multiple of 8)
  uneven    1 < nbands < tile rows, the bands differ in length (2 and 3 tile rows, or 3 and 4), and nsplit = 8 n + r with
            r > 0 (the reduce's unrolled loop AND its remainder loop)
  small     nsplit < 8 (the remainder loop alone)
All of them have a ragged last tile row (H = m th +- 1) and a ragged last tile column (W % 32 in {1, 8, 31}; the 16x16x4
fp32 kernel needs W % 4 == 0, so 8 only).  `misaligned`: fp32 with W % 4 == 0 but the slices one float off 16 bytes -- the
round-1 kernel on the band split that was planned for the 16x16x4 kernel's grid.

Checks per case (operands are channel slices at coff = 64 of NaN-filled wider buffers; dW is NaN-prefilled):
  * one-hot gy per output channel, random x:  dW[co][ci][dy][dx] == x[b_co, ci, p_co + (dy - p, dx - p)] or +0, torch.equal.
    The probe pixels sit on the image corners, on both sides of every tile-row seam (band seams first), on the first and
    last column of a tile, on the ragged last row and column, in the first, a middle and the last image.  Then the dual,
    one-hot x per input channel.  A duplicated tile shows as 2x, a dropped halo row as 0, a shifted address as a neighbour.
  * dense random data: |got - ref| <= 2^-20 S per element against float64 conv2d_weight (tests/bounds.py: assert_wgrad).
  * accumulate=True adds the same fp32 value to the prior contents: bit for bit prior + (the accumulate=False result).
Plan independence: the same images at B and, four times repeated, at 4 B run different plans; both results lie inside the
interval of the one float64 reference.

The case table itself is checked without a GPU in tests/test_bounds.py (test_wgrad_cases_cover_every_plan_class_per_form_and_dtype).
Measured max |got - ref| / S (MI355X, units of 2^-24 S): c8 bf16 0.49, fp16 0.60, f32_t16 1.56, f32 round-1 1.72 (DESIGN.md,
section 6).  GPU only."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from codon_amd import _lib as L
from tests.bounds import (WGRAD_K_CAP, assert_wgrad, wgrad_bands, wgrad_impulse_diff, wgrad_impulse_expect, wgrad_one_hot,
                          wgrad_probe_pixels, wgrad_ref)

# every (k, cin, cout) autograd.py sends to ops.conv2d_wgrad == WGRAD_CASES of test_gpu_kernels.py
FORMS = [(5, 128, 128), (5, 64, 64), (3, 64, 64), (3, 128, 64), (1, 128, 64)]
COFF = 64
_CODE = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}
_NAME = {torch.float32: "fp32", torch.bfloat16: "bf16", torch.float16: "fp16"}

# (B, H, W) per kernel family, form and plan class.  Tile heights (tests/bounds.py: WGRAD_TH16 / WGRAD_TH32 / _T16, mirrored from
# the sources): c8 10 / 6 / 4 rows for k = 5 / 3 / 1; fp32 4 (the 16x16x4 kernel's k = 1 form: 2).
_SHAPES = {
    "c8": {
        (5, 128, 128): {"one_band": (32, 41, 40), "uneven": (11, 61, 33), "small": (3, 19, 33)},
        (5, 64, 64): {"one_band": (128, 29, 40), "uneven": (65, 41, 33), "small": (3, 19, 63)},
        (3, 64, 64): {"one_band": (256, 13, 40), "uneven": (65, 49, 33), "small": (3, 11, 63)},
        (3, 128, 64): {"one_band": (128, 17, 63), "uneven": (33, 49, 33), "small": (3, 11, 40)},
        (1, 128, 64): {"one_band": (256, 11, 33), "uneven": (65, 33, 33), "small": (3, 7, 63)},
    },
    "f32_t16": {
        (5, 128, 128): {"one_band": (32, 11, 40), "uneven": (11, 25, 40), "small": (3, 7, 40)},
        (5, 64, 64): {"one_band": (128, 11, 40), "uneven": (65, 17, 40), "small": (3, 7, 40)},
        (3, 64, 64): {"one_band": (128, 11, 40), "uneven": (65, 17, 40), "small": (3, 7, 40)},
        (3, 128, 64): {"one_band": (64, 11, 40), "uneven": (13, 41, 40), "small": (3, 7, 40)},
        (1, 128, 64): {"one_band": (256, 7, 40), "uneven": (20, 53, 40), "small": (3, 3, 40)},
    },
    "f32_r1": {
        (5, 128, 128): {"one_band": (64, 11, 33), "uneven": (13, 41, 33), "small": (3, 7, 63)},
        (5, 64, 64): {"one_band": (256, 11, 33), "uneven": (129, 17, 33), "small": (3, 7, 33)},
        (3, 64, 64): {"one_band": (512, 11, 33), "uneven": (257, 17, 33), "small": (3, 7, 63)},
        (3, 128, 64): {"one_band": (256, 11, 63), "uneven": (129, 17, 63), "small": (3, 7, 33)},
        (1, 128, 64): {"one_band": (512, 11, 33), "uneven": (257, 17, 33), "small": (3, 7, 63)},
    },
}
# fp32, W % 4 == 0, slices one float off 16 bytes: the round-1 kernel on the 16x16x4 kernel's band split
_MISALIGNED = {(5, 128, 128): (11, 25, 40), (5, 64, 64): (65, 17, 40), (3, 64, 64): (65, 17, 40), (3, 128, 64): (13, 41, 40),
               (1, 128, 64): (37, 65, 40)}


def _cases():
    out = []
    for fam, dtypes in (("c8", (torch.bfloat16, torch.float16)), ("f32_t16", (torch.float32,)), ("f32_r1", (torch.float32,))):
        for dtype in dtypes:
            for form in FORMS:
                for cls, shape in _SHAPES[fam][form].items():
                    out.append(pytest.param(fam, dtype, form, cls, shape, True,
                                            id=f"{fam}-{_NAME[dtype]}-k{form[0]}_{form[1]}to{form[2]}-{cls}-{'x'.join(map(str, shape))}"))
    for form, shape in _MISALIGNED.items():
        out.append(pytest.param("f32_r1", torch.float32, form, "misaligned", shape, False,
                                id=f"f32_r1-fp32-k{form[0]}_{form[1]}to{form[2]}-misaligned-{'x'.join(map(str, shape))}"))
    for dtype in (torch.bfloat16, torch.float16):       # the training CLI's default batch: the 5x5 128 -> 128 gradient as 6 + 7 tile rows
        out.append(pytest.param("c8", dtype, (5, 128, 128), "cli_default", (16, 128, 128), True,
                                id=f"c8-{_NAME[dtype]}-k5_128to128-cli_default-16x128x128"))
    return out


def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _rand(shape, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(size=shape).astype(np.float32))


def _q(t, dtype):
    return t.to(dtype).float() if dtype != torch.float32 else t


def _buf(t, dtype, dev, aligned=True):
    """(B, C, H, W) fp32 values -> channels [COFF, COFF + C) of a NaN-filled (B, COFF + C, H, W) activation buffer of dtype
    on the device; not aligned (fp32): the buffer starts one float into its allocation."""
    from codon_amd import ops
    B, Ch, H, W = t.shape
    if dtype != torch.float32:
        full = torch.full((B, COFF + Ch, H, W), float("nan"), device=dev)
        full[:, COFF:] = t.to(dev)
        return ops.from_nchw(full, dtype)
    n = B * (COFF + Ch) * H * W
    flat = torch.full((n + 4,), float("nan"), device=dev)
    full = flat[0 if aligned else 1:][:n].view(B, COFF + Ch, H, W)
    full[:, COFF:] = t.to(dev)
    assert full.is_contiguous() and (full.data_ptr() % 16 == 0) == aligned
    return full


def _nsplit(dtype, k, cin, cout, B, H, W):
    d = L.ConvDesc(B, H, W, cin, cout, k, COFF + cin, COFF, COFF + cout, COFF, 0, 0, 0, _CODE[dtype])
    nbytes = L.load().codon_conv_wgrad_workspace_bytes(C.byref(d))
    assert nbytes > 0 and nbytes % (4 * cout * cin * k * k) == 0, nbytes
    return nbytes // (4 * cout * cin * k * k)


def _premise(fam, dtype, form, cls, shape, aligned, what):
    """The plan of this launch, read from the workspace size, checked against the restated planner and against the plan
    class the case stands for; printed."""
    k, cin, cout = form
    B, H, W = shape
    plan = wgrad_bands(dtype, k, cin, cout, B, H, W, aligned=aligned)
    nsplit = _nsplit(dtype, k, cin, cout, B, H, W)
    print(f"[plan] {what}: kernel {plan['kernel']}, nsplit {nsplit}, nbands {nsplit // B}, tile rows per band "
          f"{plan['rows_per_band']} of {plan['th']} rows, H % th = {H % plan['th']}, W % 32 = {W % 32}")
    assert nsplit == plan["nsplit"] and nsplit % B == 0, f"{what}: the library plans {nsplit} splits, the restated planner {plan['nsplit']}"
    assert plan["kernel"] == fam, (what, plan["kernel"])
    rows, nb, th = plan["rows_per_band"], plan["nbands"], plan["th"]
    assert B * H * W <= WGRAD_K_CAP
    if cls != "cli_default":
        assert W % 32 in (1, 8, 31) and (H % th in (1, th - 1)), f"{what}: ragged last tile row and column"
    if cls == "one_band":
        assert nb == 1 and rows[0] >= 3 and nsplit % 8 == 0, (what, plan)
    elif cls in ("uneven", "misaligned", "cli_default"):
        assert 1 < nb < plan["tiles"] and len(set(rows)) > 1 and max(rows) >= 2, (what, plan)
        if cls == "cli_default":
            assert rows == [6, 7] and nsplit == 32
        else:
            assert nsplit > 8 and nsplit % 8 != 0, (what, plan)
        if cls == "misaligned":                 # the split was planned for the other kernel, whose own spread differs
            t16 = wgrad_bands(dtype, k, cin, cout, B, H, W, aligned=True)
            assert t16["kernel"] == "f32_t16" and t16["nsplit"] == nsplit and t16["bands"] != plan["bands"], (what, t16, plan)
    else:
        assert cls == "small" and nsplit < 8, (what, plan)
    return plan


def _wgrad(xb, gb, cin, cout, k, dw, accumulate=False):
    from codon_amd import ops
    from codon_amd.ops import Slice
    ops.conv2d_wgrad(Slice(xb, COFF, cin), Slice(gb, COFF, cout), dw, k, accumulate=accumulate)
    torch.cuda.synchronize()
    return dw


def _untouched(bufs, what):
    from codon_amd import ops
    for b in bufs:
        assert torch.isnan(ops.to_nchw(b)[:, :COFF].float()).all(), f"{what}: an operand buffer was written"


@pytest.mark.parametrize("fam,dtype,form,cls,shape,aligned", _cases())
def test_wgrad_on_training_plans(fam, dtype, form, cls, shape, aligned):
    dev = _dev()
    k, cin, cout = form
    B, H, W = shape
    what = f"wgrad{k}x{k} {cin}->{cout} {_NAME[dtype]} {B}x{H}x{W} {cls}"
    plan = _premise(fam, dtype, form, cls, shape, aligned, what)
    seed = 1000 * k + cin + cout + B + H + W
    nan_dw = lambda: torch.full((cout, cin, k, k), float("nan"), device=dev)

    # ---- exact: one-hot gy per output channel, then one-hot x per input channel
    x = _q(_rand((B, cin, H, W), seed), dtype)
    gy = _q(_rand((B, cout, H, W), seed + 1), dtype)
    xb, gb = _buf(x, dtype, dev, aligned), _buf(gy, dtype, dev, aligned)
    for hot, n, dense in (("gy", cout, x), ("x", cin, gy)):
        for r, pix in enumerate(wgrad_probe_pixels(plan, B, H, W, n)):
            hb = _buf(wgrad_one_hot(pix, B, H, W), dtype, dev, aligned)
            got = _wgrad(xb, hb, cin, cout, k, nan_dw()) if hot == "gy" else _wgrad(hb, gb, cin, cout, k, nan_dw())
            exp = wgrad_impulse_expect(dense, pix, k, hot)
            msg = wgrad_impulse_diff(got.cpu(), exp, pix, k, hot, plan)
            assert msg is None, f"{what}, one-hot {hot}, round {r}: {msg}"
            _untouched([hb], what)

    # ---- dense: per-element float64 bound; accumulate adds the same value to the prior contents
    ref, S = wgrad_ref(x, gy, k)
    got = _wgrad(xb, gb, cin, cout, k, nan_dw())
    assert_wgrad(got, ref, S, f"{what} [{fam}]", K=B * H * W)
    prior = _rand((cout, cin, k, k), seed + 2).to(dev)
    acc = _wgrad(xb, gb, cin, cout, k, prior.clone(), accumulate=True)
    assert torch.equal(acc, prior + got), f"{what}: accumulate=True is not prior + the accumulate=False result, bit for bit"
    _untouched([xb, gb], what)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=lambda t: _NAME[t])
@pytest.mark.parametrize("k,cin,cout", FORMS)
def test_wgrad_is_plan_independent(k, cin, cout, dtype):
    """The same images at B0 and, repeated four times, at 4 B0: B0 = 64 / channel blocks runs several bands per image,
    4 B0 one band of all the tile rows.  Both results lie inside the interval of ONE float64 reference (4 ref, 4 S for the
    second: four times the same products)."""
    dev = _dev()
    H, W = 23, 40
    fam = "c8" if dtype != torch.float32 else "f32_t16"
    blocks = (cout // 64) * (cin // ({5: 32, 3: 64, 1: 128}[k] if fam == "c8" else 128 if k == 1 else 32))
    B0 = 64 // blocks
    what = f"wgrad{k}x{k} {cin}->{cout} {_NAME[dtype]} {H}x{W}"
    p1 = wgrad_bands(dtype, k, cin, cout, B0, H, W)
    p4 = wgrad_bands(dtype, k, cin, cout, 4 * B0, H, W)
    for B, p in ((B0, p1), (4 * B0, p4)):
        n = _nsplit(dtype, k, cin, cout, B, H, W)
        print(f"[plan] {what} B {B}: kernel {p['kernel']}, nsplit {n}, nbands {n // B}, tile rows per band {p['rows_per_band']}")
        assert n == p["nsplit"], (what, B, n, p)
    assert p4["nbands"] == 1 and p4["rows_per_band"][0] >= 3 and p1["nbands"] > 1, (p1, p4)
    x = _q(_rand((B0, cin, H, W), 7 * k + cin), dtype)
    gy = _q(_rand((B0, cout, H, W), 7 * k + cout + 1), dtype)
    ref, S = wgrad_ref(x, gy, k)
    for rep in (1, 4):
        xb, gb = _buf(x.repeat(rep, 1, 1, 1), dtype, dev), _buf(gy.repeat(rep, 1, 1, 1), dtype, dev)
        got = _wgrad(xb, gb, cin, cout, k, torch.full((cout, cin, k, k), float("nan"), device=dev))
        assert_wgrad(got, rep * ref, rep * S, f"{what} B {rep * B0} [{fam}]", K=rep * B0 * H * W)
