"""Non-finite input guard on the device: the stems detect NaN / +Inf / -Inf, the head poisons, the host
hears about it without a synchronisation.

The reference turns one non-finite pixel of x or y into an all-NaN map for that image and leaves the other images of the
batch bit-identical to the clean run (tests/test_nonfinite_cpu.py pins that on the oracle); here HIP is compared with HIP:
the same model's clean run is the reference for the untouched images."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import codon_oracle as orc

pytestmark = pytest.mark.gpu

NAN, PINF, NINF = float("nan"), float("inf"), float("-inf")
BAD_VALUES = (NAN, PINF, NINF)
POSITIONS = ((0, 0), (12, 20), (23, 39))
# values that must NOT trip "exponent all ones": denormals, zeros, +-FLT_MAX, negatives, the largest fp16 / bf16
FLT_MAX = float(np.finfo(np.float32).max)
NO_TRIP = (1e-45, -1e-45, 1.1754942e-38, 0.0, -0.0, FLT_MAX, -FLT_MAX, -1.0, -123456.0, 65504.0,
           float(torch.finfo(torch.bfloat16).max), -float(torch.finfo(torch.bfloat16).max))


def _rand(shape, seed):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed))


def _batch(B=3, H=24, W=40):
    """The issue's batch: torch.rand with generator seed 5 (x first, then y)."""
    g = torch.Generator().manual_seed(5)
    return torch.rand((B, 1, H, W), generator=g), torch.rand((B, 1, H, W), generator=g)


def _model(cls, sd, strict=True):
    m = cls()
    m.load_state_dict(sd, strict=strict)
    return m.cuda().eval()


def _poisoned(x, y, which, img, pos, val):
    x, y = x.clone(), y.clone()
    (x if which == "x" else y)[img, 0, pos[0], pos[1]] = val
    return x, y


def _assert_propagated(out, clean, img):
    assert out.shape == clean.shape and out.dtype == clean.dtype
    assert bool(torch.isnan(out[img]).all()), f"image {img}: {int(torch.isnan(out[img]).sum())} of {out[img].numel()} NaN"
    for b in range(out.shape[0]):
        if b != img:
            assert torch.equal(out[b], clean[b]), f"image {b} differs from the clean run"


# ---- 1. op level ------------------------------------------------------------------------------------------------------

def _stem_sweep(shape, dtype, pair):
    from codon_amd import ops
    from codon_amd.ops import Slice
    dev = torch.device("cuda", 0)
    B, _, H, W = shape
    xa, xb = _rand(shape, 11).to(dev) - 0.3, _rand(shape, 12).to(dev) - 0.3          # negatives included
    wa, wb = (torch.randn((64, 1, 3, 3), generator=torch.Generator().manual_seed(13)).to(dev),
              torch.randn((64, 1, 3, 3), generator=torch.Generator().manual_seed(14)).to(dev))
    words = torch.zeros(2, dtype=torch.int32).pin_memory()
    wnp = words.numpy()
    pa, pb = words.data_ptr(), words.data_ptr() + 4
    bad = torch.zeros(B, dtype=torch.int32, device=dev)

    def run(xa_, xb_, guarded):
        ya, yb = ops.new_act(B, 64, H, W, dtype, dev), ops.new_act(B, 64, H, W, dtype, dev)
        if pair:
            ops.stem_pair(xa_, wa, Slice(ya), xb_, wb, Slice(yb), *((bad, pa, pb) if guarded else ()))
        else:
            ops.stem(xa_, wa, Slice(ya), *((bad, pa) if guarded else ()))
            ops.stem(xb_, wb, Slice(yb), *((bad, pb) if guarded else ()))
        return ya, yb

    def check(xa_, xb_, want_bad, want_words, what):
        bad.zero_()
        wnp[:] = 0
        torch.cuda.synchronize()
        ga, gb = run(xa_, xb_, True)
        ra, rb = run(xa_, xb_, False)
        torch.cuda.synchronize()
        assert bad.cpu().tolist() == want_bad, (what, bad.cpu().tolist())
        assert wnp.tolist() == want_words, (what, wnp.tolist())
        # the stems' output bytes are the unguarded entry's
        assert torch.equal(ga.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           ra.view(torch.int16 if dtype != torch.float32 else torch.int32)), what
        assert torch.equal(gb.view(torch.int16 if dtype != torch.float32 else torch.int32),
                           rb.view(torch.int16 if dtype != torch.float32 else torch.int32)), what

    check(xa, xb, [0] * B, [0, 0], "clean")
    for v in NO_TRIP:
        t = xa.clone()
        t[:, 0, ::2, ::3] = v
        check(t, t.flip(0), [0] * B, [0, 0], f"no-trip value {v!r}")
    k = 0
    for b in range(B):
        for i in range(H):
            for j in range(W):
                val = BAD_VALUES[k % 3]
                k += 1
                inp = k % 2                                   # which input holds it
                ta, tb = xa.clone(), xb.clone()
                (ta if inp == 0 else tb)[b, 0, i, j] = val
                check(ta, tb, [1 if q == b else 0 for q in range(B)], [1, 0] if inp == 0 else [0, 1],
                      f"{val} at image {b} ({i},{j}) of input {inp}")


@pytest.mark.parametrize("pair", [False, True], ids=["stem", "stem_pair"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_stem_sweep_vec1(dtype, pair):
    """2 x 1 x 9 x 13 (W % 4 != 0: VEC 1): NaN / +Inf / -Inf at every pixel position in turn set exactly the owning image's
    word and the owning input's host word; the output bytes equal the unguarded entry's; no-trip values leave all zero."""
    _stem_sweep((2, 1, 9, 13), dtype, pair)


@pytest.mark.parametrize("pair", [False, True], ids=["stem", "stem_pair"])
def test_stem_sweep_vec4_f32(pair):
    """VEC 4 of the fp32 stems needs more than 65 536 pixels (smaller inputs take the one-pixel form): a 2 x 1 x 8 x 16 sweep
    runs VEC 1, so the four-pixel form is swept on 2 x 1 x 136 x 256 at the positions that matter to it -- the four lanes of a
    vector, vector / row / image boundaries."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dev = torch.device("cuda", 0)
    shape = (2, 1, 136, 256)
    B, _, H, W = shape
    xa, xb = _rand(shape, 21).to(dev) - 0.3, _rand(shape, 22).to(dev) - 0.3
    wa = torch.randn((64, 1, 3, 3), generator=torch.Generator().manual_seed(23)).to(dev)
    words = torch.zeros(2, dtype=torch.int32).pin_memory()
    wnp = words.numpy()
    bad = torch.zeros(B, dtype=torch.int32, device=dev)
    ya, yb, ra, rb = (torch.empty((B, 64, H, W), device=dev) for _ in range(4))
    pos = [(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (0, 255), (1, 0), (67, 129), (135, 252), (135, 255)]
    k = 0
    for b in range(B):
        for (i, j) in pos:
            val, inp = BAD_VALUES[k % 3], k % 2
            k += 1
            ta, tb = xa.clone(), xb.clone()
            (ta if inp == 0 else tb)[b, 0, i, j] = val
            bad.zero_()
            wnp[:] = 0
            torch.cuda.synchronize()
            if pair:
                ops.stem_pair(ta, wa, Slice(ya), tb, wa, Slice(yb), bad, words.data_ptr(), words.data_ptr() + 4)
                ops.stem_pair(ta, wa, Slice(ra), tb, wa, Slice(rb))
            else:
                ops.stem(ta, wa, Slice(ya), bad, words.data_ptr())
                ops.stem(tb, wa, Slice(yb), bad, words.data_ptr() + 4)
                ops.stem(ta, wa, Slice(ra))
                ops.stem(tb, wa, Slice(rb))
            torch.cuda.synchronize()
            assert bad.cpu().tolist() == [1 if q == b else 0 for q in range(B)], (b, i, j, val)
            assert wnp.tolist() == ([1, 0] if inp == 0 else [0, 1]), (b, i, j, val)
            assert torch.equal(ya.view(torch.int32), ra.view(torch.int32)) and torch.equal(yb.view(torch.int32), rb.view(torch.int32))


@pytest.mark.parametrize("pair", [False, True], ids=["stem", "stem_pair"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_stem_sweep_w16(dtype, pair):
    """2 x 1 x 8 x 16 (W % 4 == 0), every pixel position in turn.  (At this size the fp32 stems take the one-pixel form;
    the 16-bit stems own two pixels per lane at every size.)"""
    _stem_sweep((2, 1, 8, 16), dtype, pair)


def test_head_poisons_only_marked_images():
    """codon_head_fwd_guarded / _y16_guarded: bad[b] != 0 stores a quiet NaN in every element of image b; the other images
    and a NULL / all-zero `bad` give the plain entry's bits."""
    from codon_amd import ops
    from codon_amd.ops import Slice
    dev = torch.device("cuda", 0)
    for (B, H, W) in ((3, 9, 13), (3, 24, 40), (2, 136, 256)):
        f = (_rand((B, 64, H, W), 31) - 0.5).to(dev)
        w = torch.randn((1, 64, 3, 3), generator=torch.Generator().manual_seed(32)).to(dev)
        res = _rand((B, 1, H, W), 33).to(dev)
        for dtype in (torch.float32, torch.bfloat16, torch.float16):
            fx = ops.from_nchw(f, dtype)
            for odt in ((torch.float32,) if dtype == torch.float32 else (torch.float32, dtype)):
                ref, z, got = (torch.empty((B, 1, H, W), dtype=odt, device=dev) for _ in range(3))
                ops.head(Slice(fx), w, res, ref)
                bad = torch.zeros(B, dtype=torch.int32, device=dev)
                ops.head(Slice(fx), w, res, z, bad)
                bad[1] = 7
                ops.head(Slice(fx), w, res, got, bad)
                torch.cuda.synchronize()
                assert torch.equal(z, ref)
                _assert_propagated(got, ref, 1)


# ---- 2. "propagate" ---------------------------------------------------------------------------------------------------

def test_propagate_x4_f32_all_36_cases():
    from codon_amd import CODONNet
    m = _model(CODONNet, orc.he_state("x4", 0)).set_nonfinite_inputs("propagate")
    x, y = _batch()
    with torch.no_grad():
        clean = m(x.cuda(), y.cuda())
        assert bool(torch.isfinite(clean).all())
        for which in ("x", "y"):
            for pos in POSITIONS:
                for val in BAD_VALUES:
                    px, py = _poisoned(x, y, which, 1, pos, val)
                    _assert_propagated(m(px.cuda(), py.cuda()), clean, 1)
        assert torch.equal(m(x.cuda(), y.cuda()), clean)
    m.check_inputs()                                    # "propagate": nothing is ever raised


@pytest.mark.parametrize("variant,dtype", [("x4", torch.bfloat16), ("x4", torch.float16), ("x16", torch.float32),
                                           ("x16", torch.bfloat16)], ids=["x4-bf16", "x4-f16", "x16-f32", "x16-bf16"])
def test_propagate_other_precisions(variant, dtype):
    """x4 in bf16 / fp16: 16-bit inputs into the 16-bit model, the reference script's pattern (model.half() on .half() images);
    x16 in fp32 and bf16 (compute dtype)."""
    from codon_amd import CODONNet, CODONNet16
    m = _model(CODONNet if variant == "x4" else CODONNet16, orc.he_state(variant, 0)).set_nonfinite_inputs("propagate")
    x, y = _batch()
    if variant == "x4":
        m = m.to(dtype)
        x, y = x.to(dtype), y.to(dtype)
    elif dtype != torch.float32:
        m.set_compute_dtype(dtype)
    with torch.no_grad():
        clean = m(x.cuda(), y.cuda())
        assert clean.dtype == x.dtype and bool(torch.isfinite(clean).all())
        for which in ("x", "y"):
            for val in (NAN, PINF):
                px, py = _poisoned(x, y, which, 1, (12, 20), val)
                _assert_propagated(m(px.cuda(), py.cuda()), clean, 1)


@pytest.mark.parametrize("net", ["rmcr", "cross"])
def test_propagate_ablation_nets(net):
    """The two ablation nets in fp32.  The conv-only net has no global pool: on a large image the reference's NaN region is
    the pixel's receptive field, this project poisons the whole image at every size (a superset); at this
    size the receptive field IS the image (tests/test_nonfinite_cpu.py runs the oracle on it)."""
    from codon_amd import BaseNet_RMCR_fuseRMCR, BaseNet_RMCR_fuseRMCR_cross
    sd = orc.he_state("x4", 0)
    if net == "rmcr":
        m = BaseNet_RMCR_fuseRMCR()
        m.load_state_dict({k: v for k, v in sd.items() if k in m.state_dict()}, strict=True)
        m = m.cuda().eval()
    else:
        m = _model(BaseNet_RMCR_fuseRMCR_cross, sd)
    m.set_nonfinite_inputs("propagate")
    x, y = _batch()
    with torch.no_grad():
        clean = m(x.cuda(), y.cuda())
        assert bool(torch.isfinite(clean).all())
        for which in ("x", "y"):
            for val in (NAN, PINF):
                px, py = _poisoned(x, y, which, 1, (12, 20), val)
                _assert_propagated(m(px.cuda(), py.cuda()), clean, 1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_propagate_single_stem_launches_and_odd_width(dtype):
    """A batch large enough to leave the pair-launch path (two codon_stem_fwd_guarded launches) and a width with W % 4 != 0."""
    from codon_amd import CODONNet
    from codon_amd import model as M
    m = _model(CODONNet, orc.he_state("x4", 0)).set_nonfinite_inputs("propagate")
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    B, H, W = (50, 32, 62) if dtype == torch.float32 else (88, 96, 126)
    assert not M.plan_forward(B, H, W, dtype, False, False, False, True).pairs, "not past the pair-launch path"
    assert W % 4 != 0
    x, y = _rand((B, 1, H, W), 41), _rand((B, 1, H, W), 42)
    with torch.no_grad():
        clean = m(x.cuda(), y.cuda())
        img = B - 2
        px, py = _poisoned(x, y, "y", img, (H - 1, W - 1), NINF)
        _assert_propagated(m(px.cuda(), py.cuda()), clean, img)
        px, py = _poisoned(x, y, "x", 0, (0, 0), NAN)
        _assert_propagated(m(px.cuda(), py.cuda()), clean, 0)


# ---- 3. "raise" -------------------------------------------------------------------------------------------------------

def test_raise_next_forward_check_inputs_and_recovery():
    from codon_amd import CODONNet, NonFiniteInputError
    m = _model(CODONNet, orc.he_state("x4", 0))
    assert m.nonfinite_inputs == "raise"
    x, y = _batch()
    xc, yc = x.cuda(), y.cuda()
    with torch.no_grad():
        clean = m(xc, yc)
        m.check_inputs()
        for which in ("x", "y"):
            px, py = _poisoned(x, y, which, 1, (12, 20), NAN)
            out = m(px.cuda(), py.cuda())                     # enqueued: it is the NEXT call that raises
            torch.cuda.synchronize()
            _assert_propagated(out, clean, 1)                 # ... and its own map is the all-NaN one, not a finite-looking one
            with pytest.raises(NonFiniteInputError) as e:
                m(xc, yc)
            assert (e.value.depth, e.value.guidance) == (which == "x", which == "y")
            assert ("depth" in str(e.value)) == (which == "x") and ("guidance" in str(e.value)) == (which == "y")
            assert "previous forward" in str(e.value)
            assert torch.equal(m(xc, yc), clean)              # the trip was consumed: usable again, same bits
            # check_inputs() reports too (it synchronises itself)
            m(px.cuda(), py.cuda())
            with pytest.raises(NonFiniteInputError) as e:
                m.check_inputs()
            assert (e.value.depth, e.value.guidance) == (which == "x", which == "y")
            m.check_inputs()
            assert torch.equal(m(xc, yc), clean)
        # both inputs at once
        px, _ = _poisoned(x, y, "x", 0, (0, 0), PINF)
        _, py = _poisoned(x, y, "y", 2, (23, 39), NINF)
        m(px.cuda(), py.cuda())
        with pytest.raises(NonFiniteInputError) as e:
            m.check_inputs()
        assert e.value.depth and e.value.guidance
        m.check_packed()                                      # keeps its meaning: the weights are not stale


def test_raise_finds_image_31_of_32():
    from codon_amd import CODONNet, NonFiniteInputError
    m = _model(CODONNet, orc.he_state("x4", 0))
    x, y = _rand((32, 1, 16, 24), 51), _rand((32, 1, 16, 24), 52)
    with torch.no_grad():
        clean = m(x.cuda(), y.cuda())
        m.check_inputs()
        px, py = _poisoned(x, y, "x", 31, (15, 23), PINF)
        out = m(px.cuda(), py.cuda())
        with pytest.raises(NonFiniteInputError) as e:
            m.check_inputs()
        assert e.value.depth and not e.value.guidance
        _assert_propagated(out, clean, 31)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_raise_grad_mode_forward_and_nan_upstream_gradient(dtype):
    """The grad-mode forward trips as well; a backward whose upstream gradient holds a NaN trips nothing (the stencil and head
    launches of the backward are the unguarded entries: a gradient is no input of the network)."""
    from codon_amd import CODONNet, NonFiniteInputError
    m = _model(CODONNet, orc.he_state("x4", 0)).train()
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    x, y = _batch(2, 16, 24)
    xc, yc = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    out = m(xc, yc)
    assert out.requires_grad
    gy = torch.ones_like(out)
    gy[1, 0, 3, 5] = NAN
    gy[0, 0, 0, 0] = PINF
    out.backward(gy)
    torch.cuda.synchronize()
    m.check_inputs()                                          # nothing tripped
    assert xc.grad is not None
    m.zero_grad()
    px, py = _poisoned(x, y, "y", 1, (7, 11), NAN)
    out = m(px.cuda(), py.cuda())
    assert out.requires_grad and bool(torch.isnan(out[1]).all()) and bool(torch.isfinite(out[0]).all())
    with pytest.raises(NonFiniteInputError) as e:
        m.check_inputs()
    assert e.value.guidance and not e.value.depth
    m(xc.detach(), yc.detach())                               # usable again


# ---- 4. modes change nothing on finite inputs ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float16], ids=["f32", "bf16", "f16"])
def test_modes_bit_identical_on_finite_inputs(dtype):
    from codon_amd import CODONNet
    m = _model(CODONNet, orc.he_state("x4", 0))
    if dtype != torch.float32:
        m.set_compute_dtype(dtype)
    x, y = _batch()
    outs = {}
    with torch.no_grad():
        for mode in ("raise", "propagate", "ignore"):
            m.set_nonfinite_inputs(mode)
            outs[mode] = m(x.cuda(), y.cuda()).clone()
        assert torch.equal(outs["raise"], outs["ignore"]) and torch.equal(outs["propagate"], outs["ignore"])
        m.check_inputs()
        # "ignore" on a NaN input raises nothing (and detects nothing: the behaviour before the guard)
        m.set_nonfinite_inputs("ignore")
        px, py = _poisoned(x, y, "x", 1, (12, 20), NAN)
        m(px.cuda(), py.cuda())
        m.check_inputs()
        m(x.cuda(), y.cuda())
        m.set_nonfinite_inputs("raise")
        m(x.cuda(), y.cuda())
        m.check_inputs()


# ---- 5. hipGraph --------------------------------------------------------------------------------------------------------

def test_graph_raise_replay_after_bad_replay():
    from codon_amd import CODONNet, NonFiniteInputError
    from codon_amd.graph import GraphedCODON
    m = _model(CODONNet, orc.he_state("x4", 0))
    x, y = _batch()
    xc, yc = x.cuda(), y.cuda()
    with torch.no_grad():
        clean = m(xc, yc)
    g = GraphedCODON(m, xc, yc)
    assert torch.equal(g(xc, yc), clean)
    px, py = _poisoned(x, y, "y", 1, (12, 20), PINF)
    out = g(px.cuda(), py.cuda())
    torch.cuda.synchronize()
    _assert_propagated(out, clean, 1)
    with pytest.raises(NonFiniteInputError) as e:
        g(xc, yc)
    assert e.value.guidance and not e.value.depth
    assert torch.equal(g(xc, yc), clean)                      # consumed; the captured addresses are still the live ones
    m.check_inputs()


def test_graph_propagate_bad_then_good():
    """Replay bad, then good: the good output equals the eager clean bits -- the zeroing of `bad` lives inside the graph."""
    from codon_amd import CODONNet
    from codon_amd.graph import GraphedCODON
    m = _model(CODONNet, orc.he_state("x4", 0)).set_nonfinite_inputs("propagate")
    x, y = _batch()
    xc, yc = x.cuda(), y.cuda()
    with torch.no_grad():
        clean = m(xc, yc)
    g = GraphedCODON(m, xc, yc)
    for which, val in (("x", NAN), ("y", NINF)):
        px, py = _poisoned(x, y, which, 1, (12, 20), val)
        _assert_propagated(g(px.cuda(), py.cuda()), clean, 1)
        assert torch.equal(g(xc, yc), clean)
    m.check_inputs()
