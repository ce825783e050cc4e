"""Per-image range normalisation of depth codes on the MI355X.  The yardstick is the numpy restatement
tests/stretch_ref.py (pinned on the CPU by tests/test_stretch_cpu.py); the bar is EQUAL BITS throughout, no tolerance anywhere:
the three kernels over every shape, pattern and format, off the vector boundary and in place; the loops of `infer` against the
composition done by hand; and the contract of the whole path -- with the option, the depth input inference builds from a
low-resolution file is the one training builds from it.  Shapes are the smallest at which each part can go wrong: one code, less
than a run of eight, odd sizes, less and just more than one run per lane of code_range's workgroup, a batch whose second image starts
off every vector boundary."""
import math
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, metrics, train
from codon_amd.upsample import code_range, fill_holes, stretch_codes, unstretch_codes
from tests import fill_ref as F
from tests import stretch_ref as S
from tests import train_lr_ref as T

pytestmark = pytest.mark.gpu

quiet = lambda s: None                                               # noqa: E731
DEV = "cuda:0"


def _codes_dev(a):
    """numpy codes -> a device tensor: uint8, or the u16 bits as int16"""
    a = np.array(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()


def _np(t):
    a = t.cpu().numpy()
    return a.view(np.uint16) if a.dtype == np.int16 else a


def _dm(top):
    return None if top == 255 else top


# ---- the kernels against the restatement --------------------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", [f[0] for f in S.FORMATS])
@pytest.mark.parametrize("shape", S.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_equals_the_restatement(shape, fmt):
    _, _, top = next(f for f in S.FORMATS if f[0] == fmt)
    for pattern in S.PATTERNS:
        codes = S.case(shape, pattern, top)
        want, rng = S.want(shape, pattern, top)
        src = _codes_dev(codes)
        before = src.clone()
        r = code_range(src)
        assert r.dtype == torch.int32 and r.shape == (shape[0], 2) and np.array_equal(r.cpu().numpy(), rng), (shape, fmt, pattern)
        got, r2 = stretch_codes(src, _dm(top))
        assert got.shape == src.shape and got.dtype == src.dtype and got.data_ptr() != src.data_ptr() and torch.equal(r2, r)
        bad = np.argwhere(_np(got) != want)
        assert bad.size == 0, f"{shape} {fmt} {pattern}: {len(bad)} values differ, first at {bad[:3].tolist()}"
        assert torch.equal(src, before), "the argument was modified"
        back = unstretch_codes(got, r, _dm(top))
        assert np.array_equal(_np(back), S.unstretch_batch(want, rng, top))
        assert np.array_equal(_np(back)[codes != 0], codes[codes != 0])                        # the round trip of every valid code
        if pattern in ("holes", "full"):
            assert torch.equal(got, src)                             # no range / the full range: the identity
        assert torch.equal(stretch_codes(got, _dm(top))[0], got)     # idempotent


@pytest.mark.parametrize("fmt", [f[0] for f in S.FORMATS])
def test_views_off_the_vector_boundary_and_in_place(fmt):
    """A plane that starts one element into a larger buffer, as a plane of the training pool may: the same bits, nothing written
    outside it, and the same again in place."""
    _, dtype, top = next(f for f in S.FORMATS if f[0] == fmt)
    for shape in ((1, 17, 33), (3, 67, 131)):
        codes = S.case(shape, "random", top)
        want, rng = S.want(shape, "random", top)
        n = codes.size
        for lead in (1, 3):
            big = np.full(n + lead + 5, 77, dtype=dtype)
            big[lead:lead + n] = codes.reshape(-1)
            buf = _codes_dev(big)
            view = buf[lead:lead + n].view(shape)
            assert view.data_ptr() == buf.data_ptr() + lead * buf.element_size()
            r = code_range(view)
            assert np.array_equal(r.cpu().numpy(), rng)
            got, _ = stretch_codes(view, _dm(top))
            assert np.array_equal(_np(got), want)
            out, _ = stretch_codes(view, _dm(top), r, out=view)      # in place
            assert out.data_ptr() == view.data_ptr()
            after = _np(buf)
            assert np.array_equal(after[lead:lead + n].reshape(shape), want)
            assert (after[:lead] == 77).all() and (after[lead + n:] == 77).all()
            unstretch_codes(view, r, _dm(top), out=view)
            assert np.array_equal(_np(buf)[lead:lead + n].reshape(shape)[codes != 0], codes[codes != 0])


@pytest.mark.parametrize("fmt", [f[0] for f in S.FORMATS])
def test_another_planes_range_clamps(fmt):
    """The HR target of a real pair is stretched with the low-resolution map's range, which may be narrower than its own."""
    _, dtype, top = next(f for f in S.FORMATS if f[0] == fmt)
    g = np.random.default_rng(5)
    hr = g.integers(0, top + 1, size=(2, 36, 52)).astype(dtype)
    lo_hi = np.asarray([[top // 4, top // 2], [top // 3, top // 3]], dtype=np.int32)
    want, _ = S.stretch_batch(hr, top, lo_hi)
    got, r = stretch_codes(_codes_dev(hr), _dm(top), torch.from_numpy(lo_hi).cuda())
    assert np.array_equal(_np(got), want) and np.array_equal(r.cpu().numpy(), lo_hi)
    assert np.array_equal(want == 0, hr == 0) and (want[1][hr[1] != 0] == top).all()
    assert (want[0][(hr[0] != 0) & (hr[0] <= top // 4)] == 1).all() and (want[0][hr[0] >= top // 2] == top).all()
    one = stretch_codes(_codes_dev(hr[0]), _dm(top), torch.from_numpy(lo_hi[0]).cuda())[0]      # an (h, w) plane, a (2,) range
    assert one.shape == (36, 52) and np.array_equal(_np(one), want[0])
    u16 = _codes_dev(hr)
    if u16.dtype == torch.int16:                                     # uint16 tensors go the same way
        got16, _ = stretch_codes(u16.view(torch.uint16), _dm(top), torch.from_numpy(lo_hi).cuda())
        assert got16.dtype == torch.uint16 and np.array_equal(got16.view(torch.int16).cpu().numpy().view(np.uint16), want)


def test_refusals_leave_out_untouched():
    import ctypes as C
    from codon_amd import ops
    lib = L.load()
    B, h, w = 1, 5, 7
    codes = S.case((B, h, w), "random", 65535, seed=3)
    src = _codes_dev(codes)
    rng = torch.from_numpy(S.ranges(codes)).cuda()
    big = torch.full((B * h * w + 1,), -21555, dtype=torch.int16, device="cuda")
    out, keep_src, keep_rng = big[:B * h * w], src.clone(), rng.clone()
    st0 = ops._stream(torch.device(DEV))

    def call(entry, B=B, h=h, w=w, src=src.data_ptr(), bits=16, top=65535, lo_hi=rng.data_ptr(), out=out.data_ptr()):
        src = big.data_ptr() + 1 if src == "odd" else src
        lo_hi = rng.data_ptr() + 2 if lo_hi == "odd" else lo_hi
        p = lambda v: None if v is None else C.c_void_p(v)            # noqa: E731
        if entry == "code_range":
            st = lib.codon_code_range(B, h, w, p(src), bits, p(lo_hi), st0)
        else:
            st = getattr(lib, "codon_" + entry)(B, h, w, p(src), bits, top, p(lo_hi), p(out), st0)
        return st, lib.codon_last_error_string().decode()

    for entry in ("code_range", "stretch_codes", "unstretch_codes"):
        for kw, word in S.REFUSALS:
            if entry == "code_range" and ("top" in kw or "out" in kw):
                continue
            st, msg = call(entry, **kw)
            assert st == -1 and msg.startswith(entry + ": ") and word in msg, (entry, kw, msg)
            with pytest.raises(RuntimeError, match=f"{entry} failed with status -1: {entry}: "):
                L.check(st, entry)
    torch.cuda.synchronize()
    assert (big == -21555).all() and torch.equal(src, keep_src) and torch.equal(rng, keep_rng)
    assert call("stretch_codes")[0] == 0                              # and the good call they all differ from goes through
    assert np.array_equal(_np(out).reshape(B, h, w), S.stretch_batch(codes, 65535)[0]) and int(big[-1]) == -21555


def test_two_streams_same_bits():
    codes = S.case((3, 67, 131), "random", 65535)
    want, rng = S.want((3, 67, 131), "random", 65535)
    dev = _codes_dev(codes)
    torch.cuda.synchronize()
    outs = []
    for s in (torch.cuda.Stream(), torch.cuda.Stream()):
        with torch.cuda.stream(s):
            outs.append(stretch_codes(dev))
    torch.cuda.synchronize()
    for got, r in outs:
        assert np.array_equal(_np(got), want) and np.array_equal(r.cpu().numpy(), rng)


@pytest.mark.parametrize("top", [255, 10000])
def test_filling_keeps_the_range(top):
    for shape in ((3, 9, 13), (1, 70, 200)):
        for pattern in ("cross", "border", "levels", "one", "all"):
            c = _codes_dev(F.case(shape, pattern, top))
            assert torch.equal(code_range(fill_holes(c, _dm(top))), code_range(c)), (shape, pattern)


# ---- the loops of infer -----------------------------------------------------------------------------------------------------------

def _write_lr_set(root, shapes, bits, depth_max, scale=4, seed=0, extra=(1, 2)):
    """lr/ (codes in a narrow range of the grid, 6 % holes and one hole wider than the cubic's support), color/ and label/ (HR
    codes in a somewhat wider range, 5 % holes; both larger than the HR size by `extra`): (lr dir, color dir, label dir, names)."""
    g = np.random.default_rng(seed)
    top = 255 if bits == 8 else depth_max
    dirs = [os.path.join(root, n) for n in ("lr", "color", "label")]
    for d in dirs:
        os.makedirs(d)
    dt = np.uint8 if bits == 8 else np.uint16
    write = io.write_gray if bits == 8 else io.write_depth16
    names = []
    for i, (h, w) in enumerate(shapes):
        lo = top // 5 + i * (top // 50)
        lr = g.integers(lo, lo + top // 4, size=(h, w)).astype(dt)
        lr[g.uniform(size=(h, w)) < 0.06] = 0
        lr[2:h - 2, 3:w - 3] = 0
        H, W = h * scale + extra[0], w * scale + extra[1]
        lab = g.integers(max(1, lo - top // 20), lo + top // 3, size=(H, W)).astype(dt)
        lab[g.uniform(size=(H, W)) < 0.05] = 0
        names.append(f"{i:02d}.png")
        write(os.path.join(dirs[0], names[-1]), lr)
        io.write_gray(os.path.join(dirs[1], names[-1]), g.integers(0, 256, size=(H, W)).astype(np.uint8))
        write(os.path.join(dirs[2], names[-1]), lab)
    return (*dirs, names)


class _Capture:
    """Stands in for the network in run_loop: keeps the depth input it was given and returns it."""

    def __init__(self):
        self.x = []

    def __call__(self, x, y):
        self.x.append(x)
        return x


@pytest.fixture(scope="module")
def net():
    from codon_amd import CODONNet
    torch.manual_seed(5)
    return CODONNet().cuda().eval()


@pytest.mark.parametrize("fill", [False, True], ids=["holey", "filled"])
@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
def test_loop_equals_the_composition(tmp_path, net, bits, depth_max, fill):
    """run_loop(normalize=True), pipelined and serial, writes the bytes and prints the lines of
    [fill_holes ->] stretch_codes -> codes_to_input -> forward -> postprocess -> unstretch_codes done by hand, measured
    against the label's own codes."""
    lrd, cd, ld, names = _write_lr_set(str(tmp_path), [(9, 13), (10, 16)], bits, depth_max, seed=bits)
    deep = bits == 16
    dm, dmax = (depth_max if deep else None), (depth_max if deep else 65535)
    dev = torch.device(DEV)
    lines, files = [], {}
    write = io.write_depth16 if deep else io.write_gray
    hand = tmp_path / "hand"
    os.makedirs(hand)
    for f in names:
        codes, y, lab, h, w = infer._load_lr(lrd, cd, ld, f, torch.float32, 4, bits, dmax)[:5]
        c = codes.cuda()
        c = fill_holes(c, dm) if fill else c
        s, r = stretch_codes(c, dm)
        assert not torch.equal(s, c)
        with torch.no_grad():
            out = net(infer.codes_to_input(s, 4, torch.float32, dm), y.cuda())
        o = metrics.postprocess_u16(out[0, 0], depth_max) if deep else metrics.postprocess_u8(out[0, 0])
        o = unstretch_codes(o, r, dm)
        lo, hi = r.cpu().numpy()[0]
        assert lo <= int(_np(o).min()) and int(_np(o).max()) <= hi
        lab = lab.cuda()
        s_, c_ = (int(v) for v in (metrics.masked_sqerr_u16_dev if deep else metrics.masked_sqerr_dev)(lab, o).cpu())
        unit = (lambda t: metrics.codes_to_float(t) / float(depth_max)) if deep else (lambda t: t.float() / 255)   # noqa: E731
        lines.append(f"{f} {math.sqrt(s_ / c_) * 1.0 if deep else math.sqrt(s_ / c_)} {metrics.ssim(unit(lab[:h, :w]), unit(o))}")
        write(str(hand / f), o.cpu().numpy())
        files[f] = open(hand / f, "rb").read()
    kw = dict(depth_bits=bits, depth_max=dmax, lr_depth=lrd, scale=4, normalize=True, **({"fill_holes": True} if fill else {}))
    for pipelined in (False, True):
        od = tmp_path / f"out_{pipelined}"
        os.makedirs(od)
        got = []
        r = infer.run_loop(net, dev, torch.float32, None, cd, ld, str(od), pipelined=pipelined, emit=got.append, **kw)
        assert r["n"] == 2 and got == lines, (pipelined, got, lines)
        assert {f: open(od / f, "rb").read() for f in names} == files, pipelined
    got = []                                                          # and without the option the network sees other codes
    infer.run_loop(net, dev, torch.float32, None, cd, ld, None, pipelined=False, emit=got.append,
                   **{k: v for k, v in kw.items() if k != "normalize"})
    assert got != lines


@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
def test_stretched_files_give_the_same_input(tmp_path, bits, depth_max):
    """Idempotence at the level of files: a map that is already stretched reaches the network bit for bit as the map it came from."""
    lrd, cd, _, names = _write_lr_set(str(tmp_path), [(9, 13), (10, 16)], bits, depth_max, seed=3)
    top = 255 if bits == 8 else depth_max
    again = str(tmp_path / "again")
    os.makedirs(again)
    for f in names:
        c = io.read_depth_plane(os.path.join(lrd, f), bits, depth_max if bits == 16 else 65535)
        s = S.stretch(c, *S.code_range(c), top)
        assert not np.array_equal(s, c) and S.code_range(s) == (1, top)
        (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(again, f), s)
    dev = torch.device(DEV)
    xs = {}
    for d in (lrd, again):
        for pipelined in (False, True):
            m = _Capture()
            infer.run_loop(m, dev, torch.float16, None, cd, None, None, pipelined=pipelined, emit=quiet, depth_bits=bits,
                           depth_max=depth_max if bits == 16 else 65535, lr_depth=d, scale=4, normalize=True)
            xs[d, pipelined] = m.x
    first = xs[lrd, False]
    assert len(first) == 2 and all(x.dtype == torch.float16 for x in first)
    for k, v in xs.items():
        assert all(torch.equal(a, b) for a, b in zip(first, v)), k


# ---- training builds inference's input ------------------------------------------------------------------------------------------

def _d4(c, op):
    if op & 1:
        c = c.T
    if op & 2:
        c = c.flip(0)
    if op & 4:
        c = c.flip(1)
    return c


@pytest.mark.parametrize("fill", [False, True], ids=["holey", "filled"])
@pytest.mark.parametrize("bits, levels", [(8, 255), (16, 10000)])
@pytest.mark.parametrize("s", [4, 16])
def test_inference_input_is_trainings_input(tmp_path, s, bits, levels, fill):
    """TrainSet(lr_dir=, normalize=True[, fill_holes=True]): the pool is the restatement's, plane by plane -- the low-resolution
    plane (filled) stretched by its own range, the HR target stretched and clamped by THAT range, the guidance untouched -- and
    synthesize's x is the D4 window of what run_loop(lr_depth=, normalize=True) hands the network from the same file, for all
    eight ops and windows on every border."""
    recs, rows = T.case(s, levels)
    recs = [(d, g, np.where(lr > 0, levels // 6 + lr // 3, 0).astype(lr.dtype)) for d, g, lr in recs]      # a narrow range
    dd, cd, ld = T.write_set(str(tmp_path), recs, bits)
    kw = dict(depth_bits=bits, depth_max=levels if bits == 16 else 65535, lr_dir=ld, scale=s)
    ts = train.TrainSet(dd, cd, DEV, normalize=True, fill_holes=fill, **kw)
    assert ts.normalize and ts.fill_holes == fill and {r[5] for r in rows} == set(range(8))
    want = []
    for d, g, lr in recs:
        lr = F.fill_plane(lr) if fill else lr
        lo, hi = S.code_range(lr)
        assert 1 < lo < hi < levels and (d[d > 0] < lo).any() and (d > hi).any()      # the clamp is exercised
        want.append((S.stretch(d, lo, hi, levels), g, S.stretch(lr, lo, hi, levels)))
    assert np.array_equal(ts.pool.cpu().numpy(), T.pack(want, bits)[0])
    P = T.CROPS[s]
    descs = T.descs_of(rows, ts.offsets.tolist())
    train.synthesize(ts, descs, s, P)                               # the tables go up on first use
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, y, t = train.synthesize(ts, descs, s, P, **({"fill_holes": True} if fill else {}))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    m = _Capture()
    r = infer.run_loop(m, torch.device(DEV), torch.float32, None, cd, None, None, pipelined=False, emit=quiet, depth_bits=bits,
                       depth_max=levels if bits == 16 else 65535, lr_depth=ld, scale=s, normalize=True,
                       **({"fill_holes": True} if fill else {}))
    assert r["n"] == len(recs) == len(m.x)
    for b, (i, H, W, y0, x0, op) in enumerate(rows):
        whole = m.x[i][0, 0]
        assert whole.shape == (H, W)
        assert torch.equal(x[b, 0], _d4(whole[y0:y0 + P, x0:x0 + P], op)), (b, i, y0, x0, op)
    tab = torch.from_numpy(F.table(levels)).cuda()                  # and t is the window of the stretched target
    for b, (i, H, W, y0, x0, op) in enumerate(rows):
        tw = tab[torch.from_numpy(want[i][0].astype(np.int64)).cuda()]
        assert torch.equal(t[b, 0], _d4(tw[y0:y0 + P, x0:x0 + P], op)), (b, i)


def _write_holey(root, sizes, bits, depth_max, seed=0):
    """depth/ (smooth codes in a part of the grid, 6 % holes and a blob) and color/: (depth dir, color dir)."""
    g = np.random.default_rng(seed)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd)
    os.makedirs(cd)
    top = 255 if bits == 8 else depth_max
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        v = 0.4 + 0.2 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx)
        dep = np.clip(np.rint(v * top), 1, top).astype(np.uint8 if bits == 8 else np.uint16)
        gui = np.clip(v * 255 + g.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8)
        dep[g.uniform(size=(h, w)) < 0.06] = 0
        dep[2 * h // 7:4 * h // 7, 2 * w // 7:4 * w // 7] = 0
        (io.write_gray if bits == 8 else io.write_depth16)(os.path.join(dd, f"{i:02d}.png"), dep)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), gui)
    return dd, cd


@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
def test_synthetic_pool_is_the_restatement(tmp_path, bits, depth_max):
    """Without lr_dir every depth plane is stretched by its own range, wherever it starts in the byte pool; nothing else moves."""
    sizes = [(41, 47), (40, 52), (33, 35)]                          # odd sizes: 8-bit records start at odd bytes
    dd, cd = _write_holey(str(tmp_path), sizes, bits, depth_max)
    kw = dict(depth_bits=bits, depth_max=depth_max if bits == 16 else 65535)
    plain = train.TrainSet(dd, cd, DEV, **kw)
    ts = train.TrainSet(dd, cd, DEV, normalize=True, **kw)
    want = plain.pool.cpu().numpy().copy()
    top, wide = (255 if bits == 8 else depth_max), bits // 8
    assert any(o % (8 * wide) for o in plain.offsets.tolist())      # a plane off the vector boundary
    for off, (h, w) in zip(plain.offsets.tolist(), plain.sizes.tolist()):
        d = want[off:off + wide * h * w].view("<u2" if wide == 2 else np.uint8)
        lo, hi = S.code_range(d)
        assert 1 < lo < hi < top
        d[:] = S.stretch(d, lo, hi, top)
    assert np.array_equal(ts.offsets, plain.offsets) and np.array_equal(ts.pool.cpu().numpy(), want)
    assert not torch.equal(ts.pool, plain.pool)
    descs = np.asarray([[int(ts.offsets[1]), 40, 52, 3, 5, 2]], dtype=np.int64)
    for holes in (False, True):                                      # synthesize is untouched: it reads the stretched pool
        x, _, t = train.synthesize(ts, descs, 4, 32, degrade_holes=holes)
        x0, _, t0 = train.synthesize(plain, descs, 4, 32, degrade_holes=holes)
        assert not torch.equal(t, t0) and not torch.equal(x, x0)


# ---- the launches -------------------------------------------------------------------------------------------------------------------

def test_launch_sequences(tmp_path):
    """With the option an image of `infer --lr-depth` gains exactly codon_code_range and codon_stretch_codes in front of
    codon_lr_codes_to_input (behind codon_fill_holes) and codon_unstretch_codes behind the post-processing, every other call as it
    was; a training step gains nothing."""
    from tests.abi_log_8bit import _acl
    lrd, cd, ld, names = _write_lr_set(str(tmp_path / "i"), [(9, 13)], 8, 255)
    dev = torch.device(DEV)
    run = lambda **kw: infer.run_loop(_Capture(), dev, torch.float32, None, cd, ld, None, pipelined=False, emit=quiet,   # noqa: E731
                                      lr_depth=lrd, scale=4, **kw)
    run(normalize=True, fill_holes=True)                             # tables and workspace
    dd, cc = _write_holey(str(tmp_path / "t"), [(40, 48)], 8, 255)
    sets = {False: train.TrainSet(dd, cc, DEV), True: train.TrainSet(dd, cc, DEV, normalize=True)}
    descs = np.asarray([[int(sets[True].offsets[0]), 40, 48, 3, 5, k] for k in range(3)], dtype=np.int64)
    for ts in sets.values():
        train.synthesize(ts, descs, 4, 32, degrade_holes=True)
    torch.cuda.synchronize()
    real = L.load()
    logs = {}
    new = ("codon_code_range", "codon_stretch_codes", "codon_unstretch_codes")
    try:
        for key, kw in (("off", {}), ("on", {"normalize": True}), ("fill", {"fill_holes": True}),
                        ("fill_on", {"fill_holes": True, "normalize": True})):
            log = _acl().install()
            try:
                run(**kw)
            finally:
                L._lib = real
            logs[key] = [[n, a] for n, a, _ in log if n != "codon_fill_holes_workspace_bytes"]
        for key, ts in sets.items():
            log = _acl().install()
            torch.cuda.set_sync_debug_mode("error")
            try:
                train.synthesize(ts, descs, 4, 32, degrade_holes=True)
            finally:
                torch.cuda.set_sync_debug_mode("default")
                L._lib = real
            logs["train", key] = [[n, a] for n, a, _ in log]
    finally:
        L._lib = real
    names_of = lambda key: [n for n, _ in logs[key]]                  # noqa: E731
    base = names_of("off")
    assert base[:2] == ["codon_lr_codes_to_input", "codon_postprocess_u8_dt"] and not set(base) & set(new)
    assert "codon_masked_sqerr" in base and "codon_ssim_fwd" in base
    assert names_of("on") == ["codon_code_range", "codon_stretch_codes", "codon_lr_codes_to_input", "codon_postprocess_u8_dt",
                              "codon_unstretch_codes"] + base[2:]
    assert names_of("fill") == ["codon_fill_holes"] + base
    assert names_of("fill_on") == ["codon_fill_holes"] + names_of("on")
    for on, off in (("on", "off"), ("fill_on", "fill")):              # every other call with the arguments it had
        assert [c for c in logs[on] if c[0] not in new] == logs[off]
        args = {n: a for n, a in logs[on] if n in new}
        assert args["codon_code_range"][:3] == [1, 9, 13] and args["codon_code_range"][4] == 8
        assert args["codon_stretch_codes"][:3] == [1, 9, 13] and args["codon_stretch_codes"][4:6] == [8, 255]
        assert args["codon_unstretch_codes"][:3] == [1, 36, 52] and args["codon_unstretch_codes"][4:6] == [8, 255]
        assert {a[-1] for n, a in logs[on] if n in new + ("codon_lr_codes_to_input", "codon_postprocess_u8_dt")} == {"s0"}
    assert logs["train", True] == logs["train", False]                # a step costs nothing extra
    assert [n for n, _ in logs["train", False]] == ["codon_train_crops", "codon_bicubic_downsample_masked",
                                                    "codon_bicubic_upsample_masked", "codon_quantize_u8"]


# ---- the command lines ------------------------------------------------------------------------------------------------------------

def test_infer_cli_pipelined_equals_serial(tmp_path, capsys):
    from codon_amd import CODONNet
    torch.manual_seed(5)
    ck = str(tmp_path / "X4.pth")
    torch.save({"epoch": 2, "model": CODONNet()}, ck)
    for bits, depth_max, dt, more in ((8, 255, "f16", ["--self-ensemble"]), (16, 10000, "f32", ["--fill-holes"])):
        lrd, cd, ld, names = _write_lr_set(str(tmp_path / str(bits)), [(9, 13), (10, 16), (12, 11)], bits, depth_max, seed=1)
        deep = ["--depth-bits", "16", "--depth-max", str(depth_max)] if bits == 16 else []
        outs = {}
        for mode in ("serial", "pipe", "plain"):
            od = tmp_path / f"out_{bits}_{mode}"
            capsys.readouterr()
            rc = infer.main(["--scale", "4", "--lr-depth", lrd, "--input-color", cd, "--label", ld, "--out", str(od), "--weights", ck,
                             "--dtype", dt, "--report", "--bad-thresholds", "1,3", *deep, *more]
                            + (["--serial"] if mode == "serial" else []) + ([] if mode == "plain" else ["--normalize"]))
            assert rc == 0
            outs[mode] = (capsys.readouterr().out, {n: open(od / n, "rb").read() for n in names})
        assert outs["serial"] == outs["pipe"]
        assert all(outs["plain"][1][n] != outs["pipe"][1][n] for n in names)       # the option reaches the network's input
        for n in names:                                               # the written files are in the maps' own codes
            o = io.read_depth_plane(str(tmp_path / f"out_{bits}_pipe" / n), bits, depth_max if bits == 16 else 65535)
            lr = io.read_depth_plane(os.path.join(lrd, n), bits, depth_max if bits == 16 else 65535)
            if "--fill-holes" in more:
                lr = F.fill_plane(lr)
            lo, hi = S.code_range(lr)
            assert lo <= o.min() and o.max() <= hi
    capsys.readouterr()


def test_fit_resumes_bit_identically_and_keeps_the_key(tmp_path):
    dd, cd = _write_holey(str(tmp_path), [(48, 40), (40, 52), (44, 44)], 8, 255, seed=2)
    cli = lambda *extra: ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--mask-holes", "--degrade-holes", "--crop", "32",  # noqa: E731
                          "--batch", "2", "--log-every", "1", "--seed", "5", "--dtype", "bf16", *extra]
    a, b, c, d = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth", "d.pth"))
    straight = train.main(cli("--normalize", "--steps", "4", "--save", a), emit=quiet)
    train.main(cli("--normalize", "--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(cli("--normalize", "--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4] and resumed["losses"] == straight["losses"][2:]
    assert all(np.isfinite(v) for _, v in straight["losses"]) and straight["losses"][0][0] == 1
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    assert ca["args"]["normalize"] is True and cc["args"]["normalize"] is True
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    with pytest.raises(ValueError, match="normalize True != False"):
        train.main(cli("--steps", "4", "--resume", b), emit=quiet)
    off = train.main(cli("--steps", "2", "--save", d), emit=quiet)
    assert "normalize" not in torch.load(d, weights_only=False)["args"]          # a run without the option keeps its keys
    assert off["losses"] != straight["losses"][:2]
    with pytest.raises(ValueError, match="normalize False != True"):
        train.main(cli("--normalize", "--steps", "4", "--resume", d), emit=quiet)


def test_validation_normalises_as_inference_does(tmp_path, net):
    """val["normalize"] reaches run_loop through validate: the means of run_loop(lr_depth=, normalize=True) itself."""
    lrd, cd, ld, _ = _write_lr_set(str(tmp_path), [(9, 13)], 8, 255, seed=4, extra=(0, 0))
    dev = torch.device(DEV)
    val = {"lr_depth": lrd, "scale": 4, "color": cd, "label": ld, "every": 1}
    r = train.validate(net, dev, dict(val, normalize=True), emit=quiet)
    r0 = train.validate(net, dev, val, emit=quiet)
    net.eval()
    got = []
    with torch.no_grad():
        want = infer.run_loop(net, dev, torch.float32, None, cd, ld, emit=got.append, lr_depth=lrd, scale=4, normalize=True)
    assert r["n"] == 1 and (r["rmse_mean"], r["ssim_mean"]) == (want["rmse_mean"], want["ssim_mean"])
    assert got == [f"00.png {want['rmse_mean']} {want['ssim_mean']}"]
    assert (r0["rmse_mean"], r0["ssim_mean"]) != (r["rmse_mean"], r["ssim_mean"])
