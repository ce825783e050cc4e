"""The D4 self-ensemble on the MI355X.  The yardstick is the numpy restatement in tests/d4_ref.py (pinned on the
CPU by tests/test_d4_cpu.py); the bar is EQUAL BITS throughout: the views kernel copies bits (NaN payloads and -0.0 included),
the merge kernel adds in the stated tree in fp32, self_ensemble composes them around any callable, and `infer --self-ensemble`
writes what self_ensemble computes.  Shapes (B x H x W) are the smallest that reach every path of the 32 x 32 tiling: 1x5x7
below one tile, 1x32x32 exactly one, 1x33x70 across tile edges and ragged on both axes with H != W, 3x37x53 a batch."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import ensemble, infer, io, metrics
from tests import d4_ref as D

pytestmark = pytest.mark.gpu

TORCH_DT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
DTS = ("f32", "f16", "bf16")


def _to_dev(a, dt):
    """A numpy array of the dtype's BITS (or float32 / float16 values) as a device tensor of that dtype, bits untouched."""
    a = np.ascontiguousarray(a)
    carrier = {4: np.int32, 2: np.int16}[a.dtype.itemsize]
    return torch.from_numpy(a.view(carrier)).cuda().view(TORCH_DT[dt])


def _bits(t):
    """A device tensor's bits as an unsigned numpy array."""
    carrier, u = {4: (torch.int32, np.uint32), 2: (torch.int16, np.uint16)}[t.element_size()]
    return t.contiguous().view(carrier).cpu().numpy().view(u)


def _same_bits(got, ref, what):
    ref = np.asarray(ref)
    ref = ref.view({4: np.uint32, 2: np.uint16}[ref.dtype.itemsize])
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    bad = np.argwhere(got != ref)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} values differ, first at {bad[:3].tolist()}"


def _np_values(t, dt):
    """A device tensor as d4_ref.upcast takes it: float32 / float16 arrays, bf16 as uint16 bits."""
    return _bits(t) if dt == "bf16" else t.cpu().numpy()


# ---- the two kernels -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", D.SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_views_equal_the_restatement(shape, dt):
    x, y = D.random_bits(shape, dt, 1), D.random_bits(shape, dt, 2)
    B, H, W = shape
    ux, tx, uy, ty = ensemble.d4_views(_to_dev(x, dt), _to_dev(y, dt))
    assert ux.shape == uy.shape == (4 * B, 1, H, W) and tx.shape == ty.shape == (4 * B, 1, W, H) and ux.dtype == ty.dtype == TORCH_DT[dt]
    for got, ref, n in zip((ux, tx), D.views(x), ("upright x", "transposed x")):
        _same_bits(_bits(got), ref, f"{shape} {dt} {n}")
    for got, ref, n in zip((uy, ty), D.views(y), ("upright y", "transposed y")):
        _same_bits(_bits(got), ref, f"{shape} {dt} {n}")
    one = ensemble.d4_views(_to_dev(y, dt))                          # src1 = NULL: one plane only
    assert len(one) == 2
    for got, ref, n in zip(one, D.views(y), ("upright", "transposed")):
        _same_bits(_bits(got), ref, f"{shape} {dt} single plane {n}")


@pytest.mark.parametrize("shape", D.SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_merge_equals_the_restatement(shape, dt):
    """Independent random upright and transposed batches -- not views of one image, so a wrong index cannot cancel -- of
    magnitudes around 1e-3 and 1, so that the order of the adds is visible."""
    B, H, W = shape
    up, tr = D.merge_values(4 * B, H, W, dt, 3), D.merge_values(4 * B, W, H, dt, 4)
    got = ensemble.d4_merge(_to_dev(up, dt), _to_dev(tr, dt))
    assert got.dtype == torch.float32 and got.shape == (B, 1, H, W)
    ref = D.merge(D.upcast(up, dt), D.upcast(tr, dt))
    _same_bits(_bits(got), ref, f"merge {shape} {dt}")
    fu, ft = D.upcast(up, dt).astype(np.float64), D.upcast(tr, dt).astype(np.float64)
    seq = np.zeros((B, 1, H, W), dtype=np.float32)                   # the inputs do tell the tree from a running sum
    for k in range(8):
        seq = seq + np.stack([D.inverse((ft if k & 1 else fu)[4 * b + (k >> 1), 0], k) for b in range(B)])[:, None].astype(np.float32)
    assert np.any((np.float32(0.125) * seq).view(np.uint32) != ref.view(np.uint32))


# ---- self_ensemble around stand-in callables ----------------------------------------------------------------------------------------

def _ramp_t(a):
    h, w = a.shape[-2:]
    return a.float() + (torch.arange(h * w, dtype=torch.float32, device=a.device) / 64).reshape(1, 1, h, w)


@pytest.mark.parametrize("shape", D.SHAPES)
@pytest.mark.parametrize("dt", DTS)
def test_self_ensemble_with_stand_in_callables(shape, dt):
    B, H, W = shape
    x, y = D.merge_values(B, H, W, dt, 5), D.merge_values(B, H, W, dt, 6)
    xd, yd = _to_dev(x, dt), _to_dev(y, dt)
    calls = []

    def first(a, b):
        calls.append((tuple(a.shape), tuple(b.shape)))
        return a

    out = ensemble.self_ensemble(first, xd, yd)
    assert calls == [((4 * B, 1, H, W),) * 2, ((4 * B, 1, W, H),) * 2]          # two forwards of 4B views, square images included
    assert out.dtype == torch.float32 and out.shape == (B, 1, H, W)
    _same_bits(_bits(out), D.upcast(x, dt), f"{shape} {dt} model = x")          # eight equal values average to themselves
    assert torch.equal(out, xd.float())
    _same_bits(_bits(ensemble.self_ensemble(lambda a, b: b, xd, yd)), D.upcast(y, dt), f"{shape} {dt} model = y")

    # not equivariant: a position ramp sized to the callable's input, added in fp32 (the callable returns fp32)
    def ramp_np(a, b):
        h, w = a.shape[-2:]
        return D.upcast(a, dt) + (np.arange(h * w, dtype=np.float32) / np.float32(64)).reshape(1, 1, h, w)

    got = ensemble.self_ensemble(lambda a, b: _ramp_t(a), xd, yd)
    ref = D.self_ensemble(ramp_np, x, y, "f32")
    _same_bits(_bits(got), ref, f"{shape} {dt} ramp")
    assert np.abs(ref - D.upcast(x, dt)).max() > 0.05


# ---- self_ensemble around the network --------------------------------------------------------------------------------------------

def _torch_views(x):
    """The two view batches of d4_ref.views, built with ATen."""
    up, tr = [], []
    for b in range(x.shape[0]):
        for k in range(8):
            v = x[b:b + 1]
            if k & 1:
                v = v.transpose(-1, -2)
            if k & 2:
                v = v.flip(-2)
            if k & 4:
                v = v.flip(-1)
            (tr if k & 1 else up).append(v)
    return torch.cat(up).contiguous(), torch.cat(tr).contiguous()


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_self_ensemble_with_the_network(dt):
    from codon_amd import CODONNet
    torch.manual_seed(11)
    B, H, W = 1, 33, 70
    m = CODONNet().cuda().to(TORCH_DT[dt]).eval()
    g = torch.Generator().manual_seed(3)
    x = torch.rand((B, 1, H, W), generator=g).cuda().to(TORCH_DT[dt])
    y = torch.rand((B, 1, H, W), generator=g).cuda().to(TORCH_DT[dt])
    ensemble.self_ensemble(m, x, y)                                   # packed weights, tables and buffers come up on first use
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = ensemble.self_ensemble(m, x, y)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert got.dtype == torch.float32 and got.shape == (B, 1, H, W)
    (ux, tx), (uy, ty) = _torch_views(x), _torch_views(y)
    assert ux.shape == (4, 1, H, W) and tx.shape == (4, 1, W, H)
    with torch.no_grad():
        ou, ot = m(ux, uy), m(tx, ty)
    assert ou.dtype == TORCH_DT[dt]
    ref = D.merge(D.upcast(_np_values(ou, dt), dt), D.upcast(_np_values(ot, dt), dt))
    _same_bits(_bits(got), ref, f"network {dt}")
    with torch.no_grad():
        plain = m(x, y).float()
    assert not torch.equal(got, plain)                                # a random-init network is not equivariant


# ---- the infer command line ----------------------------------------------------------------------------------------------------

def _run_infer(tmp_path, capsys, tag, args):
    """infer.main pipelined and --serial: (stdout, {name: PNG bytes}) of the pipelined run, after asserting the two agree."""
    outs = {}
    for mode in ("serial", "pipe"):
        od = tmp_path / f"out_{tag}_{mode}"
        capsys.readouterr()
        assert infer.main(args + ["--out", str(od)] + (["--serial"] if mode == "serial" else [])) == 0
        outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in sorted(os.listdir(od))})
    assert outs["serial"] == outs["pipe"], tag
    return str(tmp_path / f"out_{tag}_pipe")


def test_infer_cli_self_ensemble(tmp_path, capsys):
    from codon_amd import CODONNet
    g = np.random.default_rng(8)
    dd, cd, lrd = (str(tmp_path / n) for n in ("depth", "color", "lr"))
    for d in (dd, cd, lrd):
        os.makedirs(d)
    names = []
    for i, (h, w) in enumerate([(24, 40), (40, 24)]):
        names.append(f"{i:02d}.png")
        io.write_gray(os.path.join(dd, names[-1]), g.integers(0, 256, size=(h, w)).astype(np.uint8))
        io.write_gray(os.path.join(cd, names[-1]), g.integers(0, 256, size=(h, w)).astype(np.uint8))
        lr = g.integers(1, 256, size=(h // 4, w // 4)).astype(np.uint8)          # 6 x 10 and 10 x 6 codes
        lr[1, 2] = 0                                                             # and a hole
        io.write_gray(os.path.join(lrd, names[-1]), lr)
    torch.manual_seed(6)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 1, "model": CODONNet()}, ck)
    dev = torch.device("cuda:0")

    def expect(dt, load, to_x, on):
        tdt = TORCH_DT[dt]
        m = CODONNet()
        io.load_checkpoint(ck, m)
        m = m.to(dev).to(tdt).eval()
        res = {}
        for f in names:
            x, y = load(f, tdt)[:2]
            with torch.no_grad():
                out = ensemble.self_ensemble(m, to_x(x.to(dev), tdt), y.to(dev)) if on else m(to_x(x.to(dev), tdt), y.to(dev))
            assert out.dtype == (torch.float32 if on else tdt)
            res[f] = metrics.postprocess_u8(out[0, 0]).cpu().numpy()
        return res

    hr = (lambda f, tdt: infer._load_host(dd, cd, None, f, tdt), lambda x, tdt: x, ["--input-depth", dd])
    lr4 = (lambda f, tdt: infer._load_lr(lrd, cd, None, f, tdt, 4)[:5], lambda c, tdt: infer.codes_to_input(c, 4, tdt), ["--lr-depth", lrd])
    for dt, (load, to_x, src) in [("f32", hr), ("f16", hr), ("f16", lr4)]:
        base = ["--scale", "4", "--input-color", cd, "--weights", ck, "--dtype", dt] + src
        tag = f"{dt}_{src[0].strip('-')}"
        on = _run_infer(tmp_path, capsys, tag + "_on", base + ["--self-ensemble"])
        off = _run_infer(tmp_path, capsys, tag + "_off", base)
        want_on, want_off = expect(dt, load, to_x, True), expect(dt, load, to_x, False)
        for f in names:
            got_on, got_off = io.read_gray(os.path.join(on, f)), io.read_gray(os.path.join(off, f))
            assert np.array_equal(got_on, want_on[f]), (tag, f, "with --self-ensemble")
            assert np.array_equal(got_off, want_off[f]), (tag, f, "without the flag: the plain forward's output")
            assert not np.array_equal(got_on, got_off), (tag, f)
    capsys.readouterr()


# ---- refusals --------------------------------------------------------------------------------------------------------------------

def test_self_ensemble_refusals():
    from codon_amd import CODONNet
    ident = lambda a, b: a                                                      # noqa: E731
    x = torch.zeros(1, 1, 8, 12, device="cuda")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble.self_ensemble(ident, x.cpu(), x.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ensemble.self_ensemble(ident, x, x.cpu())
    with pytest.raises(RuntimeError, match=r"two \(B,1,H,W\) tensors"):
        ensemble.self_ensemble(ident, x, x.transpose(-1, -2))
    with pytest.raises(RuntimeError, match=r"two \(B,1,H,W\) tensors"):
        ensemble.self_ensemble(ident, x[0], x[0])
    with pytest.raises(RuntimeError, match=r"two \(B,1,H,W\) tensors"):
        ensemble.self_ensemble(ident, x.expand(1, 3, 8, 12), x.expand(1, 3, 8, 12))
    for bad in (torch.float64, torch.int32, torch.uint8):
        with pytest.raises(NotImplementedError, match="not supported"):
            ensemble.self_ensemble(ident, x.to(bad), x.to(bad))
    with pytest.raises(NotImplementedError, match="not supported"):
        ensemble.self_ensemble(ident, x, x.half())
    m = CODONNet().cuda()
    assert m.training
    with pytest.raises(RuntimeError, match="training mode"):
        ensemble.self_ensemble(m, x, x)
    with pytest.raises(RuntimeError, match="the model returned"):
        ensemble.self_ensemble(lambda a, b: a[:, :, :4], x, x)
    with pytest.raises(RuntimeError, match="d4_merge expects"):
        ensemble.d4_merge(torch.zeros(4, 1, 8, 12, device="cuda"), torch.zeros(4, 1, 8, 12, device="cuda"))
    with pytest.raises(RuntimeError, match="d4_views expects"):
        ensemble.d4_views(x, x.half())
    assert ensemble.self_ensemble(ident, x[:0], x[:0]).shape == (0, 1, 8, 12)
    # nothing above left the model or the library unusable
    assert torch.equal(ensemble.self_ensemble(ident, x + 0.25, x), (x + 0.25))


def test_entry_points_refuse_bad_arguments():
    """BAD_ARG from the two C entries on NULL and on non-positive sizes, with real device pointers for the rest."""
    lib = L.load()
    t = torch.zeros(4 * 16, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert lib.codon_d4_views(1, 4, 4, None, None, L.F32, p, p, None, None, None) == -1 and b"d4_views" in lib.codon_last_error_string()
    assert lib.codon_d4_views(1, 4, 4, p, None, L.F32, None, p, None, None, None) == -1
    assert lib.codon_d4_views(1, 4, 4, p, None, L.F32, p, None, None, None, None) == -1
    assert lib.codon_d4_views(1, 4, 4, p, p, L.F32, p, p, p, None, None) == -1
    assert lib.codon_d4_views(1, 4, 4, p, None, L.F32, p, p, None, p, None) == -1
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        assert lib.codon_d4_merge(1, 4, 4, args[0], args[1], L.F32, args[2], None) == -1 and b"d4_merge" in lib.codon_last_error_string()
    for shape in ((0, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, 4, -3)):
        assert lib.codon_d4_views(*shape, p, None, L.F32, p, p, None, None, None) == -1 and b"bad shape" in lib.codon_last_error_string()
        assert lib.codon_d4_merge(*shape, p, p, L.F32, p, None) == -1 and b"bad shape" in lib.codon_last_error_string()
    assert lib.codon_d4_views(1, 4, 4, p, None, 7, p, p, None, None, None) == -1 and b"dtype" in lib.codon_last_error_string()
    assert lib.codon_d4_merge(1, 4, 4, p, p, 7, p, None) == -1 and b"dtype" in lib.codon_last_error_string()
    torch.cuda.synchronize()
    assert not t.any()                                                          # and nothing was launched
