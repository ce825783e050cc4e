"""What tests/test_gpu_gate_stencil_bounds.py rests on, checked without a GPU: the form helper's table (tests/forms.py), the
seeds of the backward cases (no hidden pre-activation on the ReLU's kink), and -- once -- that the per-element checks reject
the corruptions they exist for, applied to the float64 reference's own output at shape mid-v4 (1, 253, 260):

  one element zeroed; one column at a segment seam taken from its neighbour; the last row of a band left at NaN; one routed
  maximum sent to the second tied pixel; a result truncated toward zero to bf16.

Next to each, the verdict of the aggregate bars these kernels had before (test_gpu_kernels.py, test_gpu_backward.py,
test_gpu_c8.py: rel_rmse < 1e-6 for the stencils, < 1e-5 for g_pre, < 3e-3 for a bf16 store) is ASSERTED AS MEASURED:
  - a zeroed element passes rel_rmse < 1e-6 only while |value| < 1e-6 rms sqrt(N) (6.0e-4 at N = 65780, where nine such
    elements exist in one head output); the per-element check sees anything above tau = 2^-20 S, three orders below;
  - the bf16 truncation measures rel_rmse 3.3e-3: past the 3e-3 of one bf16 conv, inside the 1e-2 of BF16_TOL;
  - a seam column from its neighbour (rel_rmse 8.8e-2), a NaN row (NaN) and a mis-routed maximum (3.8e-2) do NOT pass the
    aggregate bars AT A SHAPE THAT RUNS THE FORM: what let them through was that no isolated test ran the form at all.
CPU only."""
import numpy as np
import pytest
import torch

from tests import cac_ref, forms
from tests.bounds import TAU_UNIT, assert_rounded, conv_ref, tau_of
from tests.test_gpu_gate_stencil_bounds import (BIG_V1, BIG_V4, BWD_SEEDS, BWD_TIES, MID_V1, MID_V4, _impulse_diff, _scatter_taps,
                                                _within, bwd_inputs)
from tests.util import rel_rmse

F32, BF16 = torch.float32, torch.bfloat16


def test_form_helper_states_the_table():
    hf = lambda dt, s: forms.head_form(dt, *s)
    assert hf(F32, (1, 64, 96))["name"] == "head<1,1,16>" and hf(F32, (1, 256, 256))["name"] == "head<1,1,16>"      # 65536: tiny
    a = hf(F32, MID_V4)
    assert a["name"] == "head<4,4,4>" and len(a["bands"]) == 64 and a["bands"][-1] == (252, 253) and a["segs"] == [(0, 256), (256, 260)]
    b = hf(F32, MID_V1)
    assert b["name"] == "head<1,4,8>" and len(b["segs"]) == 5 and b["segs"][-1] == (256, 261)
    assert forms.head_form(F32, *MID_V4, aligned=False)["name"] == "head<1,4,8>"
    c = hf(F32, BIG_V4)
    assert 4 * 1025 * 1028 >= 1 << 22 and c["name"] == "head<4,16>" and len(c["bands"]) == 65 and len(c["segs"]) == 5
    assert hf(F32, BIG_V1)["name"] == "head<1,4>" and hf(F32, (4, 1024, 1023))["name"] == "head<1,4,8>"             # below 2^22
    assert hf(BF16, MID_V4)["name"] == "head_c8<4>" and len(hf(BF16, MID_V4)["segs"]) == 5
    assert hf(torch.float16, BIG_V4)["name"] == "head_c8<8>"
    sf = lambda dt, s: forms.stem_form(dt, *s)["name"]
    assert sf(F32, MID_V4) == "stem<4>" and sf(F32, MID_V1) == "stem<1>" and sf(F32, (1, 128, 512)) == "stem<1>"      # 65536: tiny
    assert forms.stem_form(F32, *MID_V4, aligned=False)["name"] == "stem<1>" and sf(BF16, MID_V4) == "stem_c8<2>"
    assert forms.stem_form(F32, *MID_V4)["starts"][0] == (0, 3, 244)      # thread 256 of 65 vectors per row: row 3, vector 61
    s = forms.stats_form(128, 256)
    assert (s["name"], s["tile"], s["ntiles"]) == ("stats_small<256>", 256, 128)                                     # 32768: small
    s = forms.stats_form(*MID_V4[1:])
    assert (s["name"], s["ntiles"], s["last"]) == ("stats<2048,v4>", 33, 244)
    s = forms.stats_form(*MID_V1[1:])
    assert (s["name"], s["ntiles"], s["last"]) == ("stats<2048,v1>", 17, 379)
    w = forms.bwd_gate_walk(*MID_V4[1:])
    assert w["per"] == 5 and w["slices"][6:] == [(30, 33), (33, 33)]
    assert forms.bwd_gate_walk(50, 41)["slices"][:3] == [(0, 1), (1, 2), (2, 2)]
    assert forms.pack_probes([(0, 5, 5), (0, 6, 6), (0, 5, 8), (1, 5, 5)], 2, 64) == [[(0, 5, 5), (0, 5, 8), (1, 5, 5)], [(0, 6, 6)]]


@pytest.mark.parametrize("shape,quantised", [(s, False) for s in BWD_SEEDS] + [(s, True) for s in BWD_TIES],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else ("ties" if v else "continuous"))
def test_backward_seeds_keep_clear_of_the_hidden_relu(shape, quantised):
    """min |a| >= 2e-3 with the float64 pools: the GPU test asserts 1e-3 on the kernel's fp32 pools (1e-7 away)."""
    pre2, _, _, (w1, b1, w2, b2, _) = bwd_inputs(shape, BWD_SEEDS[shape], quantised)
    X = cac_ref.fcat(pre2[:, 64:], pre2[:, :64])
    ref, _ = cac_ref.gate(X, w1, b1, w2, b2)
    amin = float(ref["a"].abs().min())
    print(f"[seeds] {shape} {'ties' if quantised else ''}: min |a| = {amin:.3e}")
    assert amin >= 2e-3


# ---- sensitivity --------------------------------------------------------------------------------------------------------

def _rand(shape, seed, scale=1.0):
    return torch.from_numpy((np.random.default_rng(seed).standard_normal(size=shape) * scale).astype(np.float32))


@pytest.fixture(scope="module")
def head_mid_v4():
    """The head at mid-v4 as the float64 reference computes it, and that result stored in fp32: a correct kernel's output."""
    B, H, W = MID_V4
    f, wo, res = _rand((B, 64, H, W), 3), _rand((1, 64, 3, 3), 4, 0.1), _rand((B, 1, H, W), 5)
    ref, S = conv_ref(f, wo, 3)
    r64 = res.double()
    good = (ref + r64).float()
    check = lambda got, dtype=F32: assert_rounded(got.double(), ref, tau_of(S, r64), dtype, "head mid-v4", epi=lambda a: a + r64, S=S)
    check(good)
    return good, (ref + r64), S, check, forms.head_form(F32, B, H, W)


def _rejected(check, got, *a):
    with pytest.raises(AssertionError, match="outside"):
        check(got, *a)


def test_one_zeroed_element_is_rejected(head_mid_v4):
    good, e, S, check, _ = head_mid_v4
    N, rms = good.numel(), float(e.pow(2).mean().sqrt())
    # an ordinary element: both kinds of check see it
    bad = good.clone()
    bad[0, 0, 100, 100] = 0.0
    assert abs(float(good[0, 0, 100, 100])) > 0.1
    _rejected(check, bad)
    assert not rel_rmse(bad, e) < 1e-6
    # the largest element the aggregate bar cannot see: |v| < 1e-6 rms sqrt(N)
    blind = 0.9e-6 * rms * N ** 0.5
    cand = torch.where(good.abs() < blind, good.abs(), torch.zeros_like(good))
    i = int(cand.argmax())
    v, tau = float(good.flatten()[i]), float(tau_of(S).flatten()[i])
    print(f"[sensitivity] aggregate blind spot |v| < {blind:.2e} ({int((good.abs() < blind).sum())} elements); zeroing v = {v:.3e}, "
          f"tau there {tau:.2e}")
    assert abs(v) > 4 * tau
    bad = good.clone()
    bad.view(-1)[i] = 0.0
    assert rel_rmse(bad, e) < 1e-6                      # the old bar accepts
    _rejected(check, bad)                               # the per-element check does not


def test_a_seam_column_from_its_neighbour_is_rejected(head_mid_v4):
    good, e, _, check, form = head_mid_v4
    seam = form["segs"][1][0]
    assert seam == 256
    bad = good.clone()
    bad[..., seam] = good[..., seam - 1]
    _rejected(check, bad)
    r = rel_rmse(bad, e)
    print(f"[sensitivity] seam column from its neighbour: rel_rmse {r:.2e}")
    assert not r < 1e-6                                 # ... and so does the aggregate bar, once the form runs at all


def test_an_unwritten_band_row_is_rejected(head_mid_v4):
    good, e, _, check, form = head_mid_v4
    bad = good.clone()
    bad[0, 0, form["bands"][10][1] - 1] = float("nan")
    _rejected(check, bad)
    assert not rel_rmse(bad, e) < 1e-6                  # NaN compares false


def test_a_bf16_store_truncated_toward_zero_is_rejected(head_mid_v4):
    good, e, S, check, _ = head_mid_v4
    rn = e.float().to(BF16)
    check(rn.float(), BF16)                             # round to nearest even passes
    bits = e.float().view(torch.int32) & ~0xFFFF        # chop the low 16 bits: toward zero
    tz = bits.view(torch.float32)
    _rejected(check, tz, BF16)
    r = rel_rmse(tz, e)
    print(f"[sensitivity] bf16 truncation: rel_rmse {r:.2e}")
    assert 1e-3 < r < 4e-3                              # at the old 16-bit bars (3e-3 ... 1e-2): accepted or close to it


def test_an_impulse_on_the_wrong_side_of_a_seam_is_named(head_mid_v4):
    form = head_mid_v4[4]
    B, H, W = MID_V4
    pix = [(0, 3, 255), (0, 100, 256)]
    wo = _rand((1, 64, 3, 3), 21, 0.1)
    exp = torch.zeros((B, 1, H, W))
    _scatter_taps(exp, pix, [wo[:, c] for c in range(2)], 3)
    assert _impulse_diff(exp.clone(), exp, pix, 1, form) is None
    bad = exp.clone()
    bad[0, 0, 4, 256] = 0.0                             # the halo column of band 1, segment 1 not fetched
    msg = _impulse_diff(bad, exp, pix, 1, form)
    assert "band 1 of 64" in msg and "segment 1 of 2" in msg and "impulse at (b,h,w)=(0, 3, 255)" in msg, msg


def test_a_maximum_routed_to_the_second_tied_pixel_is_rejected():
    shape = MID_V4
    B, H, W = shape
    pre2, g_oc, _, (w1, b1, w2, b2, ws) = bwd_inputs(shape, BWD_SEEDS[shape], quantised=True)
    pre, pre_c = pre2[:, :64], pre2[:, 64:]
    X = cac_ref.fcat(pre_c, pre)
    g, _ = cac_ref.gate(X, w1, b1, w2, b2)
    pooled = torch.stack((X.max(1)[0], X.mean(1)), 1)
    s, _ = cac_ref.spatial(pooled, ws)
    # the forward's saved values as the kernels keep them: fp32
    ch, sp, pooled, pools = (t.float() for t in (g["ch"], s["sp"], pooled, g["pools"]))
    ref, S = cac_ref.backward(g_oc[:, :64], g_oc[:, 64:], pre, pre_c, ch, sp, pooled, pools, w1, b1, w2, ws)
    eq = X.flatten(2) == pools.double()[:, 1, :, None]
    fc = int((eq.sum(2) > 1)[0].nonzero()[0])           # a plane whose global maximum is tied
    second = int(eq[0, fc].nonzero()[1])
    assert int(ref["argpix"][0, fc]) == int(eq[0, fc].nonzero()[0]) != second
    argpix = ref["argpix"].clone()
    argpix[0, fc] = second
    bad, _ = cac_ref.backward(g_oc[:, :64], g_oc[:, 64:], pre, pre_c, ch, sp, pooled, pools, w1, b1, w2, ws, argpix=argpix)
    key = "g_pre_c" if fc < 64 else "g_pre"
    good = ref[key].float()
    _within(good, ref[key], TAU_UNIT * S[key], S[key], "reference stored in fp32")
    with pytest.raises(AssertionError, match="2 of"):
        _within(bad[key].float(), ref[key], TAU_UNIT * S[key], S[key], "second tied pixel")
    full = lambda d: torch.cat((d["g_pre"], d["g_pre_c"]), 1)
    r = rel_rmse(full(bad), full(ref))
    print(f"[sensitivity] global maximum of plane {fc} routed to pixel {second} instead of {int(ref['argpix'][0, fc])}: "
          f"routed term {float(ref['g_pools'][0, 1, fc]):.3e}, rel_rmse of g_pre {r:.2e}")
    assert not r < 1e-5                                 # test_gpu_backward.py's bar sees it too, at a shape with ties
