"""Every 16-bit MFMA conv form held to the correctly rounded float64 result, element by element (tests/bounds.py), and the
fp32 kernels of the same entry points to 16 fp32 units of |x| (*) |w|.  The whole-tensor RMSE bars of test_gpu_kernels.py,
test_gpu_c8.py and test_gpu_chain1x1.py dilute a handful of corrupt elements, and all but the plain bf16 conv's let a store
that truncates toward zero through (the fp16 conv, chained-conv and fp32-kernel comparisons passed against such a build);
every 16-bit case here fails on it and names the elements.

Definitions (include/codon_hip.h; R = the store rounding, a = the fp32 accumulator, m = the mask operand, y0 = the prior
contents of the output):
  codon_conv2d_fwd  plain                                y = R(a)
                    CODON_CONV_RELU                      y = R(max(a, 0))
                    CODON_CONV_ADD_RESIDUAL              y = R(a + r)
                    CODON_CONV_MASK_RELU (dgrad pack)    y = R(m > 0 ? a : 0)
                    CODON_CONV_ACCUM_OUT [+ MASK_RELU]   y = R(y0 + (m > 0 ? a : 0))     (the mask applies before the add)
                    ACCUM_OUT + MASK_RELU + MASK_SUM     y = R(m > 0 ? y0 + a : 0)
  codon_conv_chain1x1_fwd (mid materialised)             mid = R(max(a5x5, 0)),  out = R(a1x1(mid) + r)
  resident-filter conv3x3 64->64 (codon_conv_form_c8)    as codon_conv2d_fwd
The chained out is checked against the float64 1x1 of the kernel's OWN mid, so one rounding's ambiguity does not carry
into the next check.  Every operand is read from, and every result written to, a channel slice at coff = 64 of a wider
buffer whose other channels must stay untouched.

The shapes here are chosen around the 16-bit tile: at every one of them the fp32 kernels run in the cout-split form only (the
4 x 32 one-per-CU form for 1x1).  tests/test_gpu_f32_tilings.py holds the fp32 kernels to the same bound in each of their four
tilings, single and as pair grids, and compares the tilings with each other bit for bit.

Covered transitively, bit for bit, by other tests and not repeated here: the pair and mix53 launches
(test_conv_pair_is_one_launch_and_bit_identical, test_mix53_conv5x5_and_conv3x3_as_one_grid), codon_conv2d_gated_fwd /
_emit_fwd == codon_cac_apply_fwd then codon_conv2d_fwd (test_gated_conv_equals_apply_then_conv), codon_conv2d_sum_into_fwd
== conv then add (test_conv_sum_into_equals_conv_then_add), codon_conv1x1_bwd == wgrad + the masked dgrad conv
(test_conv1x1_bwd_equals_wgrad_plus_masked_dgrad).  GPU only."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from codon_amd import _lib as L
from tests.bounds import assert_rounded, conv_ref, tau_of

# every (k, cin, cout) c8_visit_shape (csrc/conv_c8.hip) lists; the set is closed under cin <-> cout, so each also runs as a dgrad launch
FORMS = [(5, 128, 128), (5, 64, 64), (3, 64, 64), (3, 128, 64), (3, 64, 128), (1, 128, 64), (1, 64, 128)]
# around the c8 tile (32 px wide, 8 rows; 16 rows for 5x5 64->64): one pixel, one row and one column past a tile on both
# axes with two images, exact tiles, and a ragged shape of three images
SHAPES = [(1, 1, 1), (2, 17, 33), (1, 16, 64), (3, 10, 37)]
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
COFF = 64
_CODE = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}


def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(size=shape) * scale).astype(np.float32))


def _q(t, dtype):
    """t rounded to dtype, as fp32 values (torch's fp32 -> 16-bit cast is one rounding to nearest even)."""
    return t.to(dtype).float() if dtype != torch.float32 else t


def _buf(t, dtype, dev):
    """(B, C, H, W) values -> channels [COFF, COFF + C) of a NaN-filled (B, COFF + C, H, W) activation buffer of dtype."""
    from codon_amd import ops
    B, Ch, H, W = t.shape
    full = torch.full((B, COFF + Ch, H, W), float("nan"))
    full[:, COFF:] = t
    return ops.from_nchw(full.to(dev), dtype)


def _read(buf, what):
    """The slice a kernel wrote, as float64 (B, C, H, W); the channels in front of it must still be NaN."""
    from codon_amd import ops
    full = ops.to_nchw(buf).double().cpu()
    assert torch.isnan(full[:, :COFF]).all(), f"{what}: channels outside the output slice were written"
    return full[:, COFF:]


def _form(B, H, W, dtype):
    d = L.ConvDesc(B, H, W, 64, 64, 3, 64, 0, 64, 0, 0, 0, 0, _CODE[dtype])
    return L.load().codon_conv_form_c8(C.byref(d))


def _variants(pack, r, m, y0):
    """(name, ops.conv2d keywords given the device slices, epilogue on float64 accumulators, additive operands, init)"""
    mask = lambda a: torch.where(m > 0, a, torch.zeros_like(a))
    if pack == L.PACK_FWD:
        return [("plain", lambda s: {}, None, (), None),
                ("relu", lambda s: dict(relu=True), torch.relu, (), None),
                ("residual", lambda s: dict(residual=s["r"]), lambda a: a + r, (r,), None)]
    return [("mask", lambda s: dict(relu_mask=s["m"]), mask, (), None),
            ("accum", lambda s: dict(accumulate=True), lambda a: y0 + a, (y0,), "y0"),
            ("accum+mask", lambda s: dict(accumulate=True, relu_mask=s["m"]), lambda a: y0 + mask(a), (y0,), "y0"),
            ("accum+mask_sum", lambda s: dict(accumulate=True, relu_mask=s["m"], mask_sum=True),
             lambda a: torch.where(m > 0, y0 + a, torch.zeros_like(a)), (y0,), "y0")]


def _check_conv(k, cin, cout, dtype, shape, seed, scale=1.0, packs=(L.PACK_FWD, L.PACK_DGRAD)):
    """One launch shape, every epilogue: x and the additive operands ~ N(0, scale^2), weights ~ N(0, 2 / (k^2 fan-out))
    given to the packer in fp32 (it rounds them itself), each conv_ref computed once and every epilogue applied to it."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dev = _dev()
    B, H, W = shape
    stats = []
    for pack in packs:
        # a dgrad launch reads dL/dy of the forward conv cout_f = cin <- cin_f = cout: its weight is (cin, cout, k, k)
        wshape = (cout, cin, k, k) if pack == L.PACK_FWD else (cin, cout, k, k)
        w = _rand(wshape, seed + 1, (2.0 / (k * k * wshape[0])) ** 0.5)
        x = _q(_rand((B, cin, H, W), seed, scale), dtype)
        r, m, y0 = (_q(_rand((B, cout, H, W), seed + j, scale), dtype) for j in (2, 3, 4))
        ref, S = conv_ref(x, _q(w, dtype), k, pack)
        wp = ops.packed_weight(w.to(dev), pack, dtype)
        xb, rb, mb = _buf(x, dtype, dev), _buf(r, dtype, dev), _buf(m, dtype, dev)
        sl = {"r": Slice(rb, COFF, cout), "m": Slice(mb, COFF, cout)}
        r64, m64, y64 = r.double(), m.double(), y0.double()
        for name, kw, epi, add, init in _variants(pack, r64, m64, y64):
            yb = _buf(y0 if init else torch.full((B, cout, H, W), float("nan")), dtype, dev)
            ops.conv2d(Slice(xb, COFF, cin), wp, Slice(yb, COFF, cout), k, **kw(sl))
            what = f"conv{k}x{k} {cin}->{cout} {str(dtype)[6:]} {B}x{H}x{W} {name}"
            stats.append(assert_rounded(_read(yb, what), ref, tau_of(S, *add), dtype, what, epi=epi, S=S))
        for b in (xb, rb, mb):                     # inputs are read-only
            assert torch.isnan(ops.to_nchw(b)[:, :COFF].float()).all()
    return stats


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t)[6:])
@pytest.mark.parametrize("k,cin,cout", FORMS)
def test_conv2d_every_epilogue_correctly_rounded(k, cin, cout, dtype):
    for i, shape in enumerate(SHAPES):
        _check_conv(k, cin, cout, dtype, shape, seed=100 * k + cin + cout + 7 * i)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda t: str(t)[6:])
def test_chain1x1_correctly_rounded(dtype):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dev = _dev()
    nan = lambda B, Ch, H, W: _buf(torch.full((B, Ch, H, W), float("nan")), dtype, dev)
    for i, (B, H, W) in enumerate(SHAPES):
        x = _q(_rand((B, 128, H, W), 40 + i), dtype)
        w5 = _rand((128, 128, 5, 5), 50 + i, (2.0 / (25 * 128)) ** 0.5)
        w1 = _rand((64, 128, 1, 1), 60 + i, (2.0 / 64) ** 0.5)
        r = _q(_rand((B, 64, H, W), 70 + i), dtype)
        xb, rb, mb, ob = _buf(x, dtype, dev), _buf(r, dtype, dev), nan(B, 128, H, W), nan(B, 64, H, W)
        ops.conv_chain1x1(Slice(xb, COFF, 128), ops.packed_weight(w5.to(dev), L.PACK_FWD, dtype),
                          ops.packed_weight(w1.to(dev), L.PACK_CHAIN1X1, dtype), Slice(ob, COFF, 64),
                          mid=Slice(mb, COFF, 128), residual=Slice(rb, COFF, 64))
        what = f"chain1x1 {str(dtype)[6:]} {B}x{H}x{W}"
        mid = _read(mb, what + " mid")
        ref5, S5 = conv_ref(x, _q(w5, dtype), 5)
        assert_rounded(mid, ref5, tau_of(S5), dtype, what + " mid", epi=torch.relu, S=S5)
        ref1, S1 = conv_ref(mid, _q(w1, dtype), 1)            # the 1x1 of the kernel's own mid
        r64 = r.double()
        assert_rounded(_read(ob, what + " out"), ref1, tau_of(S1, r64), dtype, what + " out", epi=lambda a: a + r64, S=S1)


def test_fp16_subnormals_conv3x3():
    """Inputs and epilogue operands scaled by 2^-14: about half of them, and of the outputs, are fp16 subnormals.  The
    reference script's CPU .half() keeps subnormals; so must the kernel (operands, MFMA, store)."""
    x = _q(_rand((2, 64, 17, 33), 5, 2.0 ** -14), torch.float16)
    share = float(((x != 0) & (x.abs() < 2.0 ** -14)).double().mean())
    print(f"[bounds] fp16 subnormal case: {100 * share:.1f} % of the inputs are subnormal")
    assert share > 0.4
    stats = _check_conv(3, 64, 64, torch.float16, (2, 17, 33), seed=5, scale=2.0 ** -14)
    assert all(s["exact_share"] > 0.9 for s in stats)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda t: str(t)[6:])
def test_resident_conv3x3_correctly_rounded_on_row_windows(dtype):
    """The resident-filter form (16 waves, 32 x 32 tiles, the whole filter in LDS) on a ragged 470 x 627 batch of 8, the
    forward with ReLU and the three dgrad epilogues, per element on the first and last 40 rows of images 0 and 7."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dev = _dev()
    B, H, W, R = 8, 470, 627, 40
    assert _form(B, H, W, dtype) == L.C8_FORM_RESIDENT, "the premise: a batch of 8 runs the resident-filter form"
    gen = torch.Generator(device=dev).manual_seed(11)
    nb = lambda: ops.from_nchw(torch.randn((B, 64, H, W), generator=gen, device=dev), dtype)
    x, m, y0 = nb(), nb(), nb()
    w = _rand((64, 64, 3, 3), 12, (2.0 / (9 * 64)) ** 0.5)
    wq = _q(w, dtype)
    cpu = lambda buf, b, lo, hi: ops.to_nchw(buf[b:b + 1, :, lo:hi]).double().cpu()
    refs = {}                                  # (pack, image, first row) -> (ref, S) of the window, shared by the epilogues
    for pack, name, kw, init in [(L.PACK_FWD, "relu", dict(relu=True), False),
                                 (L.PACK_DGRAD, "mask", dict(relu_mask=Slice(m)), False),
                                 (L.PACK_DGRAD, "accum", dict(accumulate=True), True),
                                 (L.PACK_DGRAD, "accum+mask_sum", dict(accumulate=True, relu_mask=Slice(m), mask_sum=True), True)]:
        y = y0.clone() if init else ops.new_act(B, 64, H, W, dtype, dev).fill_(float("nan"))
        ops.conv2d(Slice(x), ops.packed_weight(w.to(dev), pack, dtype), Slice(y), 3, **kw)
        for b in (0, B - 1):
            for r0 in (0, H - R):
                if (pack, b, r0) not in refs:
                    lo, hi = max(r0 - 1, 0), min(r0 + R + 1, H)
                    refs[pack, b, r0] = tuple(t[:, :, r0 - lo:r0 - lo + R] for t in conv_ref(cpu(x, b, lo, hi), wq, 3, pack))
                ref, S = refs[pack, b, r0]
                mw, yw = cpu(m, b, r0, r0 + R), cpu(y0, b, r0, r0 + R)
                epi = {"relu": torch.relu,
                       "mask": lambda a: torch.where(mw > 0, a, torch.zeros_like(a)),
                       "accum": lambda a: yw + a,
                       "accum+mask_sum": lambda a: torch.where(mw > 0, yw + a, torch.zeros_like(a))}[name]
                assert_rounded(cpu(y, b, r0, r0 + R), ref, tau_of(S, yw) if init else tau_of(S), dtype,
                               f"resident conv3x3 {str(dtype)[6:]} {name} image {b} rows {r0}..{r0 + R - 1}", epi=epi, S=S)
