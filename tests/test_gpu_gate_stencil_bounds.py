"""The fp32 stem / head stencils, the CAC gate forward and backward and their 16-bit twins, held to float64 element by element
in EVERY launch form (tests/forms.py asks the library for the launchers' own rules, codon_launch_form; each test asserts the
form it runs as its premise, so a threshold that moves in csrc/ fails the premise instead of moving the seams unseen).

Bound: the project's tau = 2^-20 (S + |additive operands|) of tests/bounds.py, S the same expression over absolute values
(tests/cac_ref.py for the gate); 16-bit outputs are held to the correctly rounded interval (one rounding).  Outputs are
NaN-prefilled; operands are read from, and results written to, channel slices at coff = 64 of wider NaN-filled buffers
whose other channels must stay NaN.  Every check prints a `[bounds]` line with the measured max |got - ref| / S.

Shapes: tiny = today's forms; mid-v4 (1, 253, 260) = 65780 pixels: head<4,4,4> with 64 bands (ragged last row) and 2
segments (one active lane in the second), stem<4>, the 2048-pixel stats form with 33 tiles (244 px in the last), a 33-tile
backward whose gate kernel walks slices of 5 tiles with a last slice of 3 and one empty slice; mid-v1 (2, 127, 261): head<1,4,8>
with 5 segments, stem<1> beyond tiny, the large stats form with two images and an odd H W; big-v4 / big-v1 (4, 1025, 1028 /
1027) >= 2^22 pixels: head<4,16>, head<1,4> and the 16-bit head's R = 8 form, checked on row windows.

Sigmoid outputs (ch, sp) get 8 x 2^-24 on top of the propagated tau: 1 / (1 + expf(-z)) is expf within 2 ulp, one add and
one divide on a result below 1 -- a derived 4 units, doubled; the measured excess over the propagated term is printed.

Measured on an MI355X, max |got - ref| / S against the float64 reference over all cases, in units of 2^-24 (the bound is 16;
a quarter of it, 2^-22 S = 4 units, is the line above which a value gets an explanation):
  head<1,1,16> 3.1   head<4,4,4> 5.6   head<1,4,8> 3.8   head<4,16> 4.1   head<1,4> 4.1     -- a chain of 576 fp32 fmas per
      element whose partial sums reach several times the final value; the 16-bit heads (fp32 output) measure 1.9 (R = 4) and
      2.5 (R = 8): three 192-term chains added at the end
  stem<1> 4.1   stem<4> 4.5                          -- 9 fmas; the worst elements are cancellations to a few percent of S
  conv1ch_wgrad 0.93 (one pixel) ... 0.05 (K = 65780)
  cac_stats channel mean 3.4, scaled 5.6 (128 sequential adds of products rounded first), per-tile sums 0.95, pooled mean 2.4
  cac_gate ch: never outside S_z 2^-20 / 4 alone (the propagated term is 70 - 180 units here, the sigmoid's share below 1)
  cac_spatial 2.4; at (1, 1, 1) 23 units of the single product's S / 4 = 0.13 units absolute: the sigmoid's own rounding,
      which is what the 8 x 2^-24 is for (largest excess over the propagated interval anywhere: 0.18 units, below 4)
  cac_apply 1.9   ew_sq_scale 2.0
  cac_backward g_pre 1.3, g_pre_c 1.3, db2 1.1, dw2 0.63, dw1 0.22, db1 0.15, dws 0.05  (with ties: g_pre 1.2)
16-bit stores: every element inside the correctly rounded interval; 98.7 - 100 % of them have ONE allowed value (the head's
y16 output, whose S is 576 terms wide: bf16 97 %, fp16 86 %).
No output needed a unit of its own.  GPU only."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cac_ref, forms
from tests.bounds import TAU_UNIT, assert_rounded, assert_wgrad, conv_ref, tau_of, wgrad_ref, WGRAD_K_CAP

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
_id = lambda t: str(t)[6:] if isinstance(t, torch.dtype) else "x".join(str(v) for v in t) if isinstance(t, tuple) else str(t)
COFF = 64
TINY = [(1, 1, 1), (2, 19, 45), (1, 16, 64)]
MID_V4, MID_V1 = (1, 253, 260), (2, 127, 261)
BIG_V4, BIG_V1 = (4, 1025, 1028), (4, 1025, 1027)
SIG_UNITS = 8 * 2.0 ** -24                 # see the module docstring
# seeds of the backward cases: chosen so that every hidden pre-activation has |a| >= 1e-3 (tests/test_gate_stencil_cpu.py)
BWD_SEEDS = {(2, 19, 45): 1, (1, 1, 1): 1, (2, 50, 41): 2, MID_V4: 1, MID_V1: 2}
BWD_TIES = [(2, 50, 41), MID_V4]            # also run with pre in multiples of 1/4

# unit of each cac_backward output, in multiples of S; 2^-20 unless a summation order is shown to need more
BWD_UNIT = {k: TAU_UNIT for k in ("g_pre", "g_pre_c", "dw1", "db1", "dw2", "db2", "dws")}

def _dev():
    assert torch.cuda.is_available(), "GPU test run without a GPU"
    return torch.device("cuda:0")


def _rand(shape, seed, scale=1.0):
    g = np.random.default_rng(seed)
    return torch.from_numpy((g.standard_normal(size=shape) * scale).astype(np.float32))


def _q(t, dtype):
    return t.to(dtype).float() if dtype != torch.float32 else t


def _buf(dtype, dev, *parts, shape=None):
    """NaN in channels [0, COFF), then the given (B, 64, H, W) value tensors (None: 64 NaN channels, an output) -> activation
    buffer of dtype; slice i is Slice(buf, COFF + 64 i, 64)."""
    from codon_amd import ops
    B, _, H, W = (parts[0].shape if shape is None else (shape[0], 0, shape[1], shape[2]))
    full = torch.full((B, COFF + 64 * len(parts), H, W), float("nan"))
    for i, p in enumerate(parts):
        if p is not None:
            full[:, COFF + 64 * i:COFF + 64 * (i + 1)] = p
    return ops.from_nchw(full.to(dev), dtype)


def _read(buf, what, i=0):
    """Slice i of a buffer made by _buf, as float64 (B, 64, H, W) on the CPU; the channels in front must still be NaN."""
    from codon_amd import ops
    full = ops.to_nchw(buf).double().cpu()
    assert torch.isnan(full[:, :COFF]).all(), f"{what}: channels outside the output slice were written"
    return full[:, COFF + 64 * i:COFF + 64 * (i + 1)]


def _sl(buf, i=0):
    from codon_amd.ops import Slice
    return Slice(buf, COFF + 64 * i, 64)


def _within(got, ref, bound, S, what, show=6):
    """|got - ref| <= bound per element (float64 tensors of one shape; NaN fails); prints the [bounds] line.  Returns
    max |got - ref| / S."""
    got, ref, bound, S = (t.detach().cpu().double() for t in (got, ref, bound, S))
    assert got.shape == ref.shape == bound.shape == S.shape, (what, got.shape, ref.shape, bound.shape, S.shape)
    err = (got - ref).abs()
    rel = torch.where(S > 0, err / S, err)
    worst = float(rel[~torch.isnan(rel)].max()) if got.numel() and not torch.isnan(rel).all() else float("nan")
    print(f"[bounds] {what}: {got.numel()} elements, max|got-ref|/S {worst:.3e} = {worst / 2.0 ** -24:.2f} x 2^-24")
    bad = ~(err <= bound)
    if bool(bad.any()):
        idx = bad.nonzero()[:show]
        lines = [f"  {tuple(int(v) for v in i)}: got {float(got[tuple(i)])!r} ref {float(ref[tuple(i)])!r} bound "
                 f"{float(bound[tuple(i)]):.3e} error {float(err[tuple(i)]) / max(float(S[tuple(i)]), 1e-300):.3e} S" for i in idx]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements outside the bound; first {len(idx)}:\n"
                             + "\n".join(lines))
    return worst


def _exact(got, ref, what, show=6):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bad = ~(got == ref)
    print(f"[bounds] {what}: {got.numel()} elements, exact: {int(bad.sum())} differ")
    if bool(bad.any()):
        idx = bad.nonzero()[:show]
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ from the exact value; first: "
                             + "; ".join(f"{tuple(int(v) for v in i)} got {float(got[tuple(i)])!r} expected {float(ref[tuple(i)])!r}"
                                         for i in idx))


def _sums_see_one_term(n, what):
    assert n * TAU_UNIT <= 0.25, f"{what}: {n} terms per sum: tau = 2^-20 S is more than 1/4 of a mean term (n <= {WGRAD_K_CAP})"


# ---- 1. stem ------------------------------------------------------------------------------------------------------------

_STEM_REF = {}


def _stem_case(shape):
    """x, w, the mask values (fp32, rounded per dtype by the caller) and conv_ref of both tap orders, computed once per shape."""
    if shape not in _STEM_REF:
        B, H, W = shape
        x, w = _rand((B, 1, H, W), 1), _rand((64, 1, 3, 3), 2, 0.3)
        _STEM_REF[shape] = (x, w, _rand((B, 64, H, W), 3), conv_ref(x, w, 3), conv_ref(x, w.flip(2, 3), 3))
    return _STEM_REF[shape]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", TINY + [MID_V4, MID_V1], ids=_id)
def test_stem_per_element(shape, dtype):
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    form = forms.stem_form(dtype, B, H, W)
    want = {MID_V4: "stem<4>", MID_V1: "stem<1>"}.get(shape, "stem<1>") if dtype == torch.float32 else "stem_c8<2>"
    assert form["name"] == want, (form["name"], want)
    x, w, m0, plain, flipped = _stem_case(shape)
    m = _q(m0, dtype)
    m64 = m.double()
    mb = _buf(dtype, dev, m)
    masked = lambda a: torch.where(m64 > 0, a, torch.zeros_like(a))
    for name, kw, (ref, S), epi in [("relu", dict(relu=True), plain, torch.relu),
                                    ("flip+mask", dict(flip=True, mask=_sl(mb)), flipped, masked),
                                    ("mask", dict(mask=_sl(mb)), plain, masked)]:
        yb = _buf(dtype, dev, None, shape=shape)
        ops.stencil_1to64(x.to(dev), w.to(dev), _sl(yb), **kw)
        what = f"{form['name']} {_id(dtype)} {_id(shape)} {name}"
        assert_rounded(_read(yb, what), ref, tau_of(S), dtype, what, epi=epi, S=S)
    assert torch.isnan(ops.to_nchw(mb)[:, :COFF].float()).all()


# ---- 2. head ------------------------------------------------------------------------------------------------------------

HEAD_FORMS = {(torch.float32, MID_V4): "head<4,4,4>", (torch.float32, MID_V1): "head<1,4,8>",
              (torch.float32, BIG_V4): "head<4,16>", (torch.float32, BIG_V1): "head<1,4>"}


def _head_premise(dtype, shape):
    B, H, W = shape
    form = forms.head_form(dtype, B, H, W)
    if dtype == torch.float32:
        want = HEAD_FORMS.get((dtype, shape), "head<1,1,16>")
    else:
        want = "head_c8<8>" if shape == BIG_V4 else "head_c8<4>"
    assert form["name"] == want, (form["name"], want)
    if shape == MID_V4:
        if dtype == torch.float32:
            assert len(form["bands"]) == 64 and form["bands"][-1] == (252, 253) and form["segs"] == [(0, 256), (256, 260)]
        else:
            assert len(form["segs"]) == 5
    if shape == MID_V1 and dtype == torch.float32:
        assert len(form["segs"]) == 5
    if shape == BIG_V4 and dtype == torch.float32:
        assert len(form["bands"]) == 65 and len(form["segs"]) == 5
    return form


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", TINY + [MID_V4, MID_V1], ids=_id)
def test_head_per_element(shape, dtype):
    from codon_amd import ops
    if dtype != torch.float32 and shape == MID_V1:
        shape = (2, 9, 125)          # 16-bit: mid-v1 adds no form; three 62-column segments with ONE column in the last
    dev = _dev()
    B, H, W = shape
    form = _head_premise(dtype, shape)
    f = _q(_rand((B, 64, H, W), 3), dtype)
    wo, res = _rand((1, 64, 3, 3), 4, 0.1), _rand((B, 1, H, W), 5)
    ref, S = conv_ref(f, wo, 3)
    r64 = res.double()
    fb = _buf(dtype, dev, f)
    outs = [torch.float32] + ([dtype] if dtype != torch.float32 else [])
    for ydt in outs:
        y = torch.full((B, 1, H, W), float("nan"), device=dev, dtype=ydt)
        ops.head(_sl(fb), wo.to(dev), res.to(dev), y)
        what = f"{form['name']} {_id(dtype)} {_id(shape)}" + (" y16" if ydt != torch.float32 else "")
        assert_rounded(y.double().cpu(), ref, tau_of(S, r64), ydt, what, epi=lambda a: a + r64, S=S)
    assert torch.isnan(ops.to_nchw(fb)[:, :COFF].float()).all()


def _head_windows(form, H, rows=18):
    """First `rows` rows, last `rows` rows, and `rows` rows centred on the band seam nearest the middle."""
    seam = min((a for a, _ in form["bands"][1:]), key=lambda a: abs(a - H // 2))
    return [0, seam - rows // 2, H - rows]


@pytest.mark.parametrize("dtype,shape", [(torch.float32, BIG_V4), (torch.float32, BIG_V1), (torch.bfloat16, BIG_V4),
                                         (torch.float16, BIG_V4)], ids=_id)
def test_head_big_forms_on_row_windows(dtype, shape):
    """>= 2^22 pixels: the 64-channel input is generated on the device; images 0 and B - 1 are checked over all columns on the
    first 18 rows, the last 18 rows (the ragged last band) and 18 rows across a band seam in the middle."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    R = 18
    form = _head_premise(dtype, shape)
    gen = torch.Generator(device=dev).manual_seed(17)
    full = torch.full((B, COFF + 64, H, W), float("nan"), device=dev)
    full[:, COFF:] = torch.randn((B, 64, H, W), generator=gen, device=dev)
    fb = ops.from_nchw(full, dtype)
    del full
    res = torch.randn((B, 1, H, W), generator=gen, device=dev)
    wo = _rand((1, 64, 3, 3), 4, 0.1)
    cpu = lambda buf, b, lo, hi: ops.to_nchw(buf[b:b + 1, :, lo:hi]).double().cpu()
    outs = [torch.float32] + ([dtype] if dtype != torch.float32 else [])
    ys = []
    for ydt in outs:
        y = torch.full((B, 1, H, W), float("nan"), device=dev, dtype=ydt)
        ops.head(_sl(fb), wo.to(dev), res, y)
        ys.append(y)
    wins = _head_windows(form, H, R)
    assert any(any(r0 < a < r0 + R for a, _ in form["bands"][1:]) for r0 in wins[1:2]), "the middle window crosses a band seam"
    for b in (0, B - 1):
        for r0 in wins:
            lo, hi = max(r0 - 1, 0), min(r0 + R + 1, H)
            fw = cpu(fb, b, lo, hi)
            assert torch.isnan(fw[:, :COFF]).all()
            ref, S = (t[:, :, r0 - lo:r0 - lo + R] for t in conv_ref(fw[:, COFF:], wo, 3))
            r64 = res[b:b + 1, :, r0:r0 + R].double().cpu()
            for ydt, y in zip(outs, ys):
                what = (f"{form['name']} {_id(dtype)} {_id(shape)}" + (" y16" if ydt != torch.float32 else "")
                        + f" image {b} rows {r0}..{r0 + R - 1}")
                assert_rounded(y[b:b + 1, :, r0:r0 + R].double().cpu(), ref, tau_of(S, r64), ydt, what, epi=lambda a: a + r64, S=S)
    del fb, res, ys, y
    torch.cuda.empty_cache()


# ---- 3. conv1ch_wgrad ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", TINY + [(1, 65, 130), MID_V4], ids=_id)
def test_conv1ch_wgrad_per_element(shape, dtype):
    """R[c][t] = sum_{b,q} A[b,c,q] s[b, q + (t/3 - 1, t%3 - 1)] (8-row bands, 64-pixel chunks); flip stores R[c][8 - t]."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    plan = forms.wgrad1_plan(H, W)
    if shape == (1, 65, 130):
        assert plan["bands"][-1] == (64, 65) and plan["chunks"][-1] == (128, 130)       # a ragged band and a ragged chunk
    a = _q(_rand((B, 64, H, W), 6), dtype)
    s = _rand((B, 1, H, W), 7)
    ref, S = wgrad_ref(s, a, 3)                        # dW[c][0][dy][dx] with x = s, gy = A
    ab = _buf(dtype, dev, a)
    for flip in (False, True):
        dw = torch.full((64, 1, 3, 3), float("nan"), device=dev)
        ops.conv1ch_wgrad(_sl(ab), s.to(dev), dw, flip=flip)
        got = dw.cpu().flip(2, 3) if flip else dw.cpu()
        assert_wgrad(got, ref, S, f"conv1ch_wgrad {_id(dtype)} {_id(shape)} flip={int(flip)} ({len(plan['bands'])} bands, "
                     f"{len(plan['chunks'])} chunks)", K=B * H * W)
    assert torch.isnan(ops.to_nchw(ab)[:, :COFF].float()).all()


# ---- 4 - 7. the gate forward ---------------------------------------------------------------------------------------------

STATS_FORMS = {MID_V4: ("stats<2048,v4>", 33, 244), MID_V1: ("stats<2048,v1>", 17, 379)}


def _gate_params(seed=30):
    return (_rand((8, 128), seed, 0.1), _rand((8,), seed + 1, 0.1), _rand((64, 8), seed + 2, 0.3), _rand((64,), seed + 3, 0.1),
            _rand((1, 2, 5, 5), seed + 4, 0.2))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", TINY + [MID_V4, MID_V1], ids=_id)
def test_cac_stats_and_gate_per_element(shape, dtype):
    """cac_stats / cac_stats_scaled: channel max and per-tile maxima exact, channel mean and per-tile sums within tau;
    cac_gate on the kernel's own partials: pooled mean within tau, pooled max exact, ch against the float64 MLP + sigmoid
    of the kernel's OWN pools within S_z 2^-20 / 4 + 8 x 2^-24."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    form = forms.stats_form(H, W)
    name, nt, last = STATS_FORMS.get(shape, ("stats_small<256>", None, None))
    assert form["name"] == name and (nt is None or (form["ntiles"], form["last"]) == (nt, last)), form
    assert form["ntiles"] == ops.cac_stats_tiles(H, W)
    nt = form["ntiles"]
    _sums_see_one_term(max(form["tile"], 128), "cac_stats")
    pre_c, pre = _q(_rand((B, 64, H, W), 8), dtype), _q(_rand((B, 64, H, W), 9), dtype)
    chs = torch.rand((B, 64), generator=torch.Generator().manual_seed(10))
    pcb, pdb = _buf(dtype, dev, pre_c), _buf(dtype, dev, pre)
    tag = f"{form['name']} {_id(dtype)} {_id(shape)}"
    partials = None
    for scaled in (True, False):                       # the plain pass last: its partials feed the gate below
        ref, S = cac_ref.stats(pre_c, pre, form["tile"], chs if scaled else None)
        pooled = torch.full((B, 2, H, W), float("nan"), device=dev)
        partials = torch.full((B, nt, 128, 2), float("nan"), device=dev)
        if scaled:
            ops.cac_stats_scaled(_sl(pcb), _sl(pdb), chs.to(dev), pooled, partials)
        else:
            ops.cac_stats(_sl(pcb), _sl(pdb), pooled, partials)
        t = tag + (" scaled" if scaled else "")
        _exact(pooled[:, 0], ref["chmax"], t + " channel max")
        _exact(partials[..., 1], ref["tile_max"], t + " per-tile maxima")
        _within(pooled[:, 1], ref["chmean"], TAU_UNIT * S["chmean"], S["chmean"], t + " channel mean")
        _within(partials[..., 0], ref["tile_sum"], TAU_UNIT * S["tile_sum"], S["tile_sum"], t + " per-tile sums")
    for b in (pcb, pdb):
        assert torch.isnan(ops.to_nchw(b)[:, :COFF].float()).all()
    # the gate, on the kernel's own partials
    w1, b1, w2, b2, _ = _gate_params()
    ch = torch.full((B, 64), float("nan"), device=dev)
    pools = torch.full((B, 2, 128), float("nan"), device=dev)
    ops.cac_gate(B, H, W, partials, *(p.to(dev) for p in (w1, b1, w2, b2)), ch, pools)
    pref, pS = cac_ref.pools_of(partials, H * W)
    _sums_see_one_term(nt, "cac_gate")
    _within(pools[:, 0], pref[:, 0], TAU_UNIT * pS[:, 0], pS[:, 0], tag + " pooled mean")
    _exact(pools[:, 1], pref[:, 1], tag + " pooled max")
    mref, mS = cac_ref.mlp(pools, w1, b1, w2, b2)
    first = TAU_UNIT * mS["z"] / 4
    _within(ch, mref["ch"], first + SIG_UNITS, mS["z"] / 4, tag + " ch")
    excess = float(((ch.double().cpu() - mref["ch"]).abs() - first).max())
    print(f"[bounds] {tag} ch: measured excess over S_z 2^-20 / 4: {excess / 2.0 ** -24:+.2f} x 2^-24 (allowed 8)")


@pytest.mark.parametrize("shape", TINY + [(1, 33, 70), MID_V1], ids=_id)
def test_cac_spatial_per_element(shape):
    """sp = sigmoid(conv5x5_{2->1}(pooled)), 32 x 32 tiles with a 2-pixel halo: the float64 sigmoid is monotone, so the
    correctly rounded interval applies as is, widened by 8 x 2^-24 for expf, the add and the divide."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    tiles = forms.spatial_tiles(H, W)
    if shape == (1, 33, 70):
        assert tiles["rows"][-1] == (32, 33) and tiles["cols"][-1] == (64, 70)
    pooled, ws = _rand((B, 2, H, W), 11), _gate_params()[4]
    ref, S = conv_ref(pooled, ws, 5)
    sp = torch.full((B, 1, H, W), float("nan"), device=dev)
    ops.cac_spatial(pooled.to(dev), ws.to(dev), sp)
    what = f"cac_spatial {_id(shape)} ({len(tiles['rows'])} x {len(tiles['cols'])} tiles)"
    tau = tau_of(S)
    got = sp.double().cpu()
    lo, hi = torch.sigmoid(ref - tau) - SIG_UNITS, torch.sigmoid(ref + tau) + SIG_UNITS
    e = torch.sigmoid(ref)
    worst = float(((got - e).abs() / (S / 4)).max())
    excess = float(torch.maximum(got - torch.sigmoid(ref + tau), torch.sigmoid(ref - tau) - got).max())
    print(f"[bounds] {what}: {got.numel()} elements, max|got-ref|/S {worst:.3e} (S = S_z / 4); excess over the propagated "
          f"interval {excess / 2.0 ** -24:+.2f} x 2^-24 (allowed 8)")
    bad = ~((got >= lo) & (got <= hi))
    assert not bool(bad.any()), (what, int(bad.sum()), [tuple(int(v) for v in i) for i in bad.nonzero()[:6]])


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("shape", TINY + [MID_V4, MID_V1], ids=_id)
def test_cac_apply_and_sq_scale_per_element(shape, dtype):
    """out = pre ch sp + inputs for both streams (two multiplies and an add) within 2^-20 (|pre ch sp| + |inputs|);
    ew_sq_scale y = x x ch within 2^-20 |x x ch|; 16-bit stores correctly rounded."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    pre, pre_c, inp, inp_c = (_q(_rand((B, 64, H, W), 12 + i), dtype) for i in range(4))
    g = torch.Generator().manual_seed(16)
    ch, sp = torch.rand((B, 64), generator=g), torch.rand((B, 1, H, W), generator=g)
    pb, ib = _buf(dtype, dev, pre, pre_c), _buf(dtype, dev, inp, inp_c)
    ob = _buf(dtype, dev, None, None, shape=shape)
    ops.cac_apply(_sl(pb, 0), _sl(pb, 1), ch.to(dev), sp.to(dev), _sl(ib, 0), _sl(ib, 1), _sl(ob, 0), _sl(ob, 1))
    tag = f"{_id(dtype)} {_id(shape)} ({-(-H * W // forms.PX_TILE)} tiles)"
    for i, (p, q, nm) in enumerate([(pre, inp, "out"), (pre_c, inp_c, "out_c")]):
        ref, S = cac_ref.apply(p, ch, sp, q)
        assert_rounded(_read(ob, nm, i), ref, TAU_UNIT * S, dtype, f"cac_apply {nm} {tag}", S=S)
    yb = _buf(dtype, dev, None, shape=shape)
    ops.ew_sq_scale(_sl(pb, 1), ch.to(dev), _sl(yb))
    ref, S = cac_ref.sq_scale(pre_c, ch)
    assert_rounded(_read(yb, "ew_sq_scale"), ref, TAU_UNIT * S, dtype, f"ew_sq_scale {tag}", S=S)
    for b in (pb, ib):
        assert torch.isnan(ops.to_nchw(b)[:, :COFF].float()).all()


# ---- 8. the gate backward -----------------------------------------------------------------------------------------------

def bwd_inputs(shape, seed, quantised=False):
    """The operands of a backward case (CPU fp32): pre2 = [pre | pre_c], g_oc = [g_out | g_out_c], base (the running gradient
    of the inputs) and the gate parameters.  quantised: pre2 in multiples of 1/4 -- ties in all three max-routings."""
    B, H, W = shape
    pre2 = _rand((B, 128, H, W), seed)
    if quantised:
        pre2 = torch.round(pre2 * 4) / 4
    return pre2, _rand((B, 128, H, W), seed + 100), _rand((B, 128, H, W), seed + 200), _gate_params(seed + 300)


@pytest.mark.parametrize("accumulate_in", [False, True], ids=["store", "accumulate"])
@pytest.mark.parametrize("shape,quantised", [((2, 19, 45), False), ((1, 1, 1), False), ((2, 50, 41), False), (MID_V4, False),
                                             (MID_V1, False)] + [(s, True) for s in BWD_TIES], ids=_id)
def test_cac_backward_per_element(shape, quantised, accumulate_in):
    """cac_backward (fp32) against tests/cac_ref.py's analytic backward on the operands the kernels were given -- the fp32
    forward's own ch, sp, pooled, pools -- every output within 2^-20 S per element.  The routed maxima are O(1) outliers of
    g_pre: a wrong first-pixel or first-channel choice is far outside tau, and with pre in multiples of 1/4 ties are common.
    g_in with accumulation is one fp32 add: equal to torch's.  The hidden ReLU's derivative is discontinuous: the seeds are
    such that every hidden pre-activation has |a| >= 1e-3 (asserted: a condition on the inputs, not a tolerance)."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    walk = forms.bwd_gate_walk(H, W)
    if shape == (2, 50, 41):
        assert (walk["ntiles"], walk["last"]) == (2, 2)
    if shape == MID_V4:
        assert walk["ntiles"] == 33 and walk["slices"] == [(0, 5), (5, 10), (10, 15), (15, 20), (20, 25), (25, 30), (30, 33), (33, 33)]
    if shape == MID_V1:
        assert walk["ntiles"] == 17 and walk["per"] == 3 and walk["slices"][5:] == [(15, 17), (17, 17), (17, 17)]
    _sums_see_one_term(forms.PX_TILE, "cac_backward per-tile sums")
    pre2, g_oc, base, (w1, b1, w2, b2, ws) = bwd_inputs(shape, BWD_SEEDS[shape], quantised)
    f32 = torch.float32
    pb, gb = _buf(f32, dev, pre2[:, :64], pre2[:, 64:]), _buf(f32, dev, g_oc[:, :64], g_oc[:, 64:])
    nt = ops.cac_stats_tiles(H, W)
    pooled, partials = torch.empty((B, 2, H, W), device=dev), torch.empty((B, nt, 128, 2), device=dev)
    ch, sp, pools = torch.empty((B, 64), device=dev), torch.empty((B, 1, H, W), device=dev), torch.empty((B, 2, 128), device=dev)
    d = lambda t: t.to(dev)
    ops.cac_stats(_sl(pb, 1), _sl(pb, 0), pooled, partials)
    ops.cac_gate(B, H, W, partials, d(w1), d(b1), d(w2), d(b2), ch, pools)
    ops.cac_spatial(pooled, d(ws), sp)
    gpb = _buf(f32, dev, None, None, shape=shape)
    gib = _buf(f32, dev, base[:, :64], base[:, 64:]) if accumulate_in else _buf(f32, dev, None, None, shape=shape)
    outs = ops.cac_backward(_sl(gb, 0), _sl(gb, 1), _sl(pb, 0), _sl(pb, 1), ch, sp, pooled, pools, d(w1), d(b1), d(w2), d(ws),
                            _sl(gpb, 0), _sl(gpb, 1), _sl(gib, 0), _sl(gib, 1), accumulate_in=accumulate_in)
    ref, S = cac_ref.backward(g_oc[:, :64], g_oc[:, 64:], pre2[:, :64], pre2[:, 64:], ch, sp, pooled, pools, w1, b1, w2, ws)
    amin = float(ref["a"].abs().min())
    print(f"[bounds] cac_backward {_id(shape)}: min |hidden pre-activation| {amin:.3e}; {walk['ntiles']} tiles, slices of {walk['per']}")
    assert amin >= 1e-3, "the case sits on the hidden ReLU's kink: choose another seed"
    if quantised:
        X = cac_ref.fcat(pre2[:, 64:], pre2[:, :64])
        ties_c = float(((X == pooled.double().cpu()[:, :1]).sum(1) > 1).double().mean())
        ties_p = float(((X.flatten(2) == pools.double().cpu()[:, 1, :, None]).sum(2) > 1).double().mean())
        print(f"[bounds] cac_backward {_id(shape)} ties: channel max at {100 * ties_c:.0f} % of the pixels, global max at "
              f"{100 * ties_p:.0f} % of the planes")
        assert ties_c > 0.1 and ties_p > 0.1
    tag = f"cac_backward {_id(shape)}{' ties' if quantised else ''} {'accumulate' if accumulate_in else 'store'}"
    got = {"g_pre": _read(gpb, tag, 0), "g_pre_c": _read(gpb, tag, 1)}
    got.update({k: v for k, v in zip(("dw1", "db1", "dw2", "db2", "dws"), outs)})
    for k, v in got.items():
        _within(v, ref[k], BWD_UNIT[k] * S[k], S[k], f"{tag} {k}")
    gi = _read(gib, tag, 0), _read(gib, tag, 1)
    for i, nm in enumerate(("g_in", "g_in_c")):
        go = g_oc[:, 64 * i:64 * (i + 1)]
        want = base[:, 64 * i:64 * (i + 1)] + go if accumulate_in else go              # torch's fp32 add: correctly rounded
        _exact(gi[i], want, f"{tag} {nm}")
    for b in (pb, gb):
        assert torch.isnan(ops.to_nchw(b)[:, :COFF].float()).all()


# ---- 9. impulses --------------------------------------------------------------------------------------------------------

def _impulse_diff(got, exp, pix, reach, form, rows_key="bands", cols_key="segs", show=6):
    """None when got == exp bit for bit (B, C, H, W), else a message naming the first wrong output pixels, the probe each
    belongs to and that probe's band and segment under `form`."""
    if torch.equal(got, exp):
        return None
    bad = (got != exp) | torch.isnan(got)
    lines = []
    for b, c, h, w in bad.nonzero()[:show].tolist():
        near = [p for p in pix if p[0] == b and abs(p[1] - h) <= reach and abs(p[2] - w) <= reach]
        src = (f"impulse at (b,h,w)={near[0]}: {forms.where(form, near[0][1], near[0][2], rows_key, cols_key)}" if near
               else "no impulse nearby")
        lines.append(f"  output (b,c,h,w)=({b}, {c}, {h}, {w}) [{forms.where(form, h, w, rows_key, cols_key)}]: got "
                     f"{float(got[b, c, h, w])!r} expected {float(exp[b, c, h, w])!r}; {src}")
    return f"{int(bad.sum())} of {got.numel()} elements differ from the exact one-hot result; first {len(lines)}:\n" + "\n".join(lines)


def _scatter_taps(exp, pix, vals, k):
    """exp[b, :, h + p - dy, w + p - dx] = vals[i][:, dy, dx] for probe i = (b, h, w), p = k // 2 (inside the image)."""
    B, _, H, W = exp.shape
    p = k // 2
    for i, (b, h, w) in enumerate(pix):
        for dy in range(k):
            for dx in range(k):
                hh, ww = h + p - dy, w + p - dx
                if 0 <= hh < H and 0 <= ww < W:
                    exp[b, :, hh, ww] = vals[i][:, dy, dx]


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (2, 19, 45)), (torch.float32, MID_V4), (torch.float32, MID_V1),
                                         (torch.bfloat16, MID_V4), (torch.float16, (2, 19, 45))], ids=_id)
def test_stem_impulses(dtype, shape):
    """x = 1.0 at probe pixels (3 x 3 footprints disjoint), 0 elsewhere: y[b, co, h + 1 - dy, w + 1 - dx] = w[co][dy][dx],
    a gather with no arithmetic -- bit for bit, for the plain and the flipped tap order."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    form = forms.stem_form(dtype, B, H, W)
    rows = [(0, 1), (1, H - 1), (H - 1, H)] if H > 2 else [(0, H)]
    pix = forms.probe_pixels(B, H, W, rows, form["segs"])
    for (b, h, w) in form["starts"]:                     # both sides of a workgroup's first thread
        pix += [(b, h, w), (b, h, w - 1) if w > 0 else (b, h - 1, W - 1) if h > 0 else (b, h, w)]
    w = _q(_rand((64, 1, 3, 3), 2, 0.3), dtype)          # representable in the output type: the store is exact
    for flip in (False, True):
        for rnd in forms.pack_probes(pix, 2, 4096):
            x = torch.zeros((B, 1, H, W))
            for (b, h, ww) in rnd:
                x[b, 0, h, ww] = 1.0
            yb = _buf(dtype, dev, None, shape=shape)
            ops.stencil_1to64(x.to(dev), w.to(dev), _sl(yb), flip=flip)
            exp = torch.zeros((B, 64, H, W), dtype=torch.float64)
            _scatter_taps(exp, rnd, [(w.flip(2, 3) if flip else w)[:, 0].double()] * len(rnd), 3)
            msg = _impulse_diff(_read(yb, "stem impulses"), exp, rnd, 1, dict(form, bands=[(r, r + 1) for r in range(H)]))
            assert msg is None, f"{form['name']} {_id(dtype)} {_id(shape)} flip={int(flip)}: {msg}"
    print(f"[bounds] {form['name']} {_id(dtype)} {_id(shape)} impulses: {len(set(pix))} probes, exact")


@pytest.mark.parametrize("dtype,shape", [(torch.float32, (2, 19, 45)), (torch.float32, MID_V4), (torch.float32, MID_V1),
                                         (torch.float32, BIG_V4), (torch.float32, BIG_V1), (torch.bfloat16, MID_V4),
                                         (torch.float16, (2, 19, 45)), (torch.bfloat16, BIG_V4)], ids=_id)
def test_head_impulses(dtype, shape):
    """Channel c of the input is 1.0 at probe pixel c (3 x 3 footprints disjoint) and 0 elsewhere, res = 0:
    y[b, 0, h + 1 - dy, w + 1 - dx] = w[c][dy][dx] -- bit for bit.  Probes: the four corners, both sides of EVERY band seam
    and of every segment seam, the ragged last row and column."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    form = _head_premise(dtype, shape)
    rows, cols = forms.seam_lines(form["bands"], H), forms.seam_lines(form["segs"], W)
    pix = [(0, 0, 0), (B - 1, 0, W - 1), (0, H - 1, 0), (B - 1, H - 1, W - 1)]
    pix += [((B - 1) * (i % 2), h, cols[i % len(cols)]) for i, h in enumerate(rows)]
    some = [rows[0], rows[len(rows) // 2], rows[-1]] + [r for r in rows if r in (form["rows"] - 1, form["rows"])]
    pix += [((B - 1) * ((i + j) % 2), h, w) for i, w in enumerate(cols) for j, h in enumerate(dict.fromkeys(some))]
    pix = list(dict.fromkeys(pix))
    wo = _rand((1, 64, 3, 3), 21, 0.1)
    full = torch.full((B, COFF + 64, H, W), float("nan"), device=dev)
    full[:, COFF:] = 0
    res = torch.zeros((B, 1, H, W), device=dev)
    for rnd in forms.pack_probes(pix, 2, 64):
        idx = tuple(torch.tensor(v, device=dev) for v in zip(*[(b, COFF + c, h, w) for c, (b, h, w) in enumerate(rnd)]))
        full[idx] = 1.0
        y = torch.full((B, 1, H, W), float("nan"), device=dev)
        ops.head(_sl(ops.from_nchw(full, dtype)), wo.to(dev), res, y)
        full[idx] = 0.0
        exp = torch.zeros((B, 1, H, W))
        _scatter_taps(exp, rnd, [wo[:, c] for c in range(len(rnd))], 3)
        msg = _impulse_diff(y.cpu(), exp, rnd, 1, form)
        assert msg is None, f"{form['name']} {_id(dtype)} {_id(shape)}: {msg}"
    print(f"[bounds] {form['name']} {_id(dtype)} {_id(shape)} impulses: {len(pix)} probes over {len(form['bands'])} bands x "
          f"{len(form['segs'])} segments, exact")
    del full, res, y
    torch.cuda.empty_cache()


@pytest.mark.parametrize("shape", [(2, 19, 45), (1, 33, 70), MID_V1], ids=_id)
def test_cac_spatial_impulses(shape):
    """pooled = 1.0 at probe pixels (plane i % 2; 5 x 5 footprints disjoint): the logit at (h + 2 - dy, w + 2 - dx) is
    ws[plane][dy][dx] exactly, 0 elsewhere, so sp must equal -- bit for bit -- the kernel's own sigmoid of that weight (taken
    from an impulse in the middle of a 5 x 5 image, itself held to the float64 sigmoid within 8 x 2^-24) and 0.5 elsewhere."""
    from codon_amd import ops
    dev = _dev()
    B, H, W = shape
    ws = _gate_params()[4]
    cal = torch.zeros((2, 2, 5, 5))
    cal[0, 0, 2, 2] = cal[1, 1, 2, 2] = 1.0
    out = torch.full((2, 1, 5, 5), float("nan"), device=dev)
    ops.cac_spatial(cal.to(dev), ws.to(dev), out)
    table = out.cpu()[:, 0].flip(1, 2)                   # table[plane][dy][dx] = the kernel's sigmoid(ws[0][plane][dy][dx])
    dev64 = (table.double() - torch.sigmoid(ws[0].double())).abs().max()
    print(f"[bounds] cac_spatial sigmoid of the 50 weights: max |got - float64| {float(dev64) / 2.0 ** -24:.2f} x 2^-24 (allowed 8)")
    assert float(dev64) <= SIG_UNITS
    tiles = forms.spatial_tiles(H, W)
    form = {"bands": tiles["rows"], "segs": tiles["cols"]}
    pix = forms.probe_pixels(B, H, W, tiles["rows"], tiles["cols"])
    for rnd in forms.pack_probes(pix, 4, 4096):
        pooled = torch.zeros((B, 2, H, W))
        for i, (b, h, w) in enumerate(rnd):
            pooled[b, i % 2, h, w] = 1.0
        sp = torch.full((B, 1, H, W), float("nan"), device=dev)
        ops.cac_spatial(pooled.to(dev), ws.to(dev), sp)
        exp = torch.full((B, 1, H, W), 0.5)
        _scatter_taps(exp, rnd, [table[i % 2][None] for i in range(len(rnd))], 5)
        msg = _impulse_diff(sp.cpu(), exp, rnd, 2, form)
        assert msg is None, f"cac_spatial {_id(shape)}: {msg}"
    print(f"[bounds] cac_spatial {_id(shape)} impulses: {len(pix)} probes over {len(tiles['rows'])} x {len(tiles['cols'])} tiles, exact")
