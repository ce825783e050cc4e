"""tests/cac_ref.py is a REFERENCE, not a second opinion: fed the float64 forward's own ch, sp, pooled and pools, its analytic
backward equals torch.autograd of the oracle's CAC gate (oracle.codon_oracle.cac_channel / cac_spatial) in float64 to
1e-12 per element -- with continuous values and with values quantised to multiples of 1/4, where ties in all three
max-routings are everywhere (torch routes a maximum to its first occurrence, as the kernel states).  CPU only."""
import numpy as np
import pytest
import torch

from oracle import codon_oracle as orc
from tests import cac_ref

REL = 1e-12
SHAPES = [(2, 19, 45), (1, 5, 3)]


def _rand(shape, seed, scale=1.0):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(size=shape) * scale)      # float64


def _case(shape, quantised, seed=0):
    B, H, W = shape
    q = (lambda t: torch.round(t * 4) / 4) if quantised else (lambda t: t)
    pre2 = q(_rand((B, 128, H, W), seed + 1))                     # [pre | pre_c]
    in2 = q(_rand((B, 128, H, W), seed + 2))
    g_oc = q(_rand((B, 128, H, W), seed + 8))
    par = [_rand((8, 128), seed + 3, 0.1), _rand((8,), seed + 4, 0.1), _rand((64, 8), seed + 5, 0.3), _rand((64,), seed + 6, 0.1),
           _rand((1, 2, 5, 5), seed + 7, 0.2)]
    return pre2, in2, g_oc, par


def _close(got, ref, S, what):
    """|got - ref| <= 1e-12 S per element, S the element's own absolute-value sum (the scale of every per-element bound of
    this project, tests/bounds.py).  Relative to |ref| itself the two float64 evaluations cannot agree to 1e-12 everywhere:
    an element whose terms cancel to 1e-5 S carries the 1e-16 S rounding noise of two different summation orders as 1e-11
    of its value (measured: 2.4e-12 at (2, 19, 45)); that figure is printed, the one against S is asserted.  A wrong route
    or a missing term is an error of order S."""
    err = (got - ref).abs()
    rel_s = float((err / S.clamp_min(1e-300)).max())
    rel_v = float((err / ref.abs().clamp_min(1e-300)).max())
    print(f"[cac_ref] {what}: max |difference| / S {rel_s:.2e}, / |value| {rel_v:.2e}")
    assert bool((err <= REL * S).all()), (what, rel_s)


@pytest.mark.parametrize("quantised", [False, True], ids=["continuous", "ties"])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_reference_equals_float64_autograd_of_the_oracle(shape, quantised):
    B, H, W = shape
    pre2, in2, g_oc, par = _case(shape, quantised)
    pre2.requires_grad_(True)
    w1, b1, w2, b2, ws = (p.requires_grad_(True) for p in par)
    pre, pre_c = pre2[:, :64], pre2[:, 64:]
    Fc = torch.cat((pre_c, pre), 1)
    ch = orc.cac_channel(Fc, w1, b1, w2, b2)
    sp = orc.cac_spatial(Fc, ws)
    g = ch[:, :, None, None] * sp
    out = torch.cat((pre * g + in2[:, :64], pre_c * g + in2[:, 64:]), 1)
    out.backward(g_oc)

    # the float64 forward of cac_ref itself: equal to the oracle's, and the operands of the backward
    d = lambda t: t.detach()
    st, _ = cac_ref.stats(d(pre_c), d(pre), tile=256)
    gt, Sg = cac_ref.gate(d(Fc), d(w1), d(b1), d(w2), d(b2))
    gp, _ = cac_ref.gate(torch.stack((st["tile_sum"], st["tile_max"]), 3), d(w1), d(b1), d(w2), d(b2), HW=H * W)
    pooled = torch.stack((st["chmax"], st["chmean"]), 1)
    s_, Ss = cac_ref.spatial(pooled, d(ws))
    _close(gt["ch"], d(ch), Sg["ch"], "ch")
    _close(gp["ch"], d(ch), Sg["ch"], "ch from per-tile partials")
    assert torch.equal(gp["pools"][:, 1], gt["pools"][:, 1])
    _close(s_["sp"], d(sp), Ss["sp"], "sp")
    o, So = cac_ref.apply(d(pre), gt["ch"], s_["sp"], in2[:, :64])
    _close(o, d(out[:, :64]), So, "out")
    if quantised:
        X = d(Fc)
        ties_c = float(((X == pooled[:, :1]).sum(1) > 1).double().mean())
        ties_p = float(((X.flatten(2) == gt["pools"][:, 1, :, None]).sum(2) > 1).double().mean())
        print(f"[cac_ref] ties: channel max tied at {100 * ties_c:.0f} % of the pixels, global max at {100 * ties_p:.0f} % of the planes")
        assert ties_c > 0.1 and ties_p > 0.1                 # the premise of this case: ties are common

    ref, S = cac_ref.backward(g_oc[:, :64], g_oc[:, 64:], d(pre), d(pre_c), gt["ch"], s_["sp"], pooled, gt["pools"],
                              d(w1), d(b1), d(w2), d(ws))
    auto = {"g_pre": pre2.grad[:, :64], "g_pre_c": pre2.grad[:, 64:], "dw1": w1.grad, "db1": b1.grad, "dw2": w2.grad,
            "db2": b2.grad, "dws": ws.grad}
    for k, v in auto.items():
        _close(ref[k], v, S[k], k)
        assert bool((S[k] >= ref[k].abs() * (1 - 1e-12)).all()), k          # S bounds the value it belongs to


def test_reference_forward_partials_tile_by_tile():
    """stats(): a tile is `tile` consecutive pixels of the flattened plane, the last one ragged; the scaled form's maxima are
    those of the fp32-rounded products."""
    B, H, W = 2, 7, 9                                  # 63 pixels: tiles of 16 -> 4 tiles, the last of 15
    pre2 = _rand((B, 128, H, W), 3).float().double()
    ref, S = cac_ref.stats(pre2[:, 64:], pre2[:, :64], tile=16)
    X = torch.cat((pre2[:, 64:], pre2[:, :64]), 1).flatten(2)
    assert tuple(ref["tile_sum"].shape) == (B, 4, 128)
    for t in range(4):
        seg = X[:, :, 16 * t:16 * t + 16]
        assert torch.allclose(ref["tile_sum"][:, t], seg.sum(2), rtol=0, atol=1e-12)
        assert torch.equal(ref["tile_max"][:, t], seg.max(2)[0])
        assert torch.allclose(S["tile_sum"][:, t], seg.abs().sum(2), rtol=0, atol=1e-12)
    chs = torch.rand((B, 64), dtype=torch.float32)
    rs, _ = cac_ref.stats(pre2[:, 64:], pre2[:, :64], tile=16, chs=chs)
    prod = (X.float() * chs.repeat(1, 2)[:, :, None]).double()          # one fp32 multiply
    assert torch.equal(rs["chmax"].flatten(1), prod.max(1)[0])
    assert torch.equal(rs["tile_max"][:, 3], prod[:, :, 48:].max(2)[0])
