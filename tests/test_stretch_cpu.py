"""The per-image range normalisation without a GPU: what the definition promises, asserted on the numpy restatement
(tests/stretch_ref.py) -- exhaustively over every range of the 8-bit grid, and for u16 codes with depth_max 65535 and 10000 over
random ranges and the extremes n = 0, n = 1, n = T; the shared cases; the refusals of the three C entries, of the Python
functions and of the command lines; and a resume of a checkpoint written before the option existed."""
import ctypes as C
import dataclasses
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, train
from tests import stretch_ref as S


def _check_range(lo, hi, top):
    """Every promise of the definition for one range, over all of [lo, hi] (and the clamp over the whole grid's ends)."""
    c = np.arange(lo, hi + 1, dtype=np.int64)
    s = S.stretch(c, lo, hi, top)
    assert s[0] == (1 if hi > lo else top) and s[-1] == top          # the range's ends land on the grid's ends
    assert np.all(np.diff(s) >= 1)                                   # monotone and injective
    assert s.min() >= 1                                              # a valid code never becomes a hole
    assert np.array_equal(S.unstretch(s, lo, hi, top), c)            # the round trip is exact
    u = S.unstretch(np.asarray([0, 1, top], dtype=np.int64), lo, hi, top)
    assert u.tolist() == [lo, lo, hi]                                # output 0 and 1 -> lo, top -> hi: always inside [lo, hi]
    out = np.asarray([0, 1, max(lo - 1, 1), hi + 1 if hi < top else top, top], dtype=np.int64)
    t = S.stretch(out, lo, hi, top)                                  # another plane's codes are clamped into the range
    assert t[0] == 0 and t[1] == s[0] and t[2] == s[0] and t[3] == top and t[4] == top


def test_every_range_of_the_8bit_grid():
    for lo in range(1, 256):
        for hi in range(lo, 256):
            _check_range(lo, hi, 255)


@pytest.mark.parametrize("top", [65535, 10000])
def test_u16_ranges(top):
    T = top - 1
    g = np.random.default_rng(top)
    pairs = [(1, top), (1, 1), (top, top), (7, 7), (1, 2), (top - 1, top), (top // 2, top // 2 + 1), (2, top), (1, top - 1)]
    for _ in range(40):
        lo = int(g.integers(1, top + 1))
        pairs.append((lo, int(g.integers(lo, top + 1))))
    assert {hi - lo for lo, hi in pairs} >= {0, 1, T}
    for lo, hi in pairs:
        _check_range(lo, hi, top)
    # the product 2 k T needs 64 bits at the top of the 16-bit grid
    assert 2 * 65534 * 65534 > 2 ** 32 and S.stretch(np.asarray([65535], dtype=np.uint16), 1, 65535, 65535)[0] == 65535


@pytest.mark.parametrize("top", [255, 65535, 10000])
def test_identity_idempotence_and_holes(top):
    g = np.random.default_rng(3)
    c = g.integers(0, top + 1, size=(5, 9)).astype(np.uint8 if top == 255 else np.uint16)
    c[0, 0], c[1, 1], c[2, 2] = 1, top, 0
    assert S.code_range(c) == (1, top)
    assert np.array_equal(S.stretch(c, 1, top, top), c)              # the full range: the identity
    d = (c.astype(np.int64) // 3 + (c > 0) * (top // 5)).astype(c.dtype)
    lo, hi = S.code_range(d)
    assert 1 < lo < hi < top
    s = S.stretch(d, lo, hi, top)
    assert s.dtype == d.dtype and np.array_equal(s == 0, d == 0)     # holes stay holes, nothing else becomes one
    assert S.code_range(s) == (1, top)
    assert np.array_equal(S.stretch(s, *S.code_range(s), top), s)    # hence idempotent
    assert np.array_equal(S.unstretch(s, lo, hi, top)[d > 0], d[d > 0])
    z = np.zeros((3, 4), dtype=c.dtype)
    assert S.code_range(z) == (0, 0)
    for bad in ((0, 0), (0, 5), (5, 4), (3, top + 1)):               # no range: both maps are the identity
        assert np.array_equal(S.stretch(d, *bad, top), d) and np.array_equal(S.unstretch(d, *bad, top), d)


def test_shared_cases_are_what_they_say():
    for name, dtype, top in S.FORMATS:
        for shape in S.SHAPES:
            ranges = {p: S.want(shape, p, top)[1] for p in S.PATTERNS}
            assert ranges["holes"].tolist() == [[0, 0]] * shape[0]
            assert all(lo == hi > 0 for lo, hi in ranges["one"]) and all(lo == hi > 0 for lo, hi in ranges["constant"])
            assert np.array_equal(S.want(shape, "full", top)[0], S.case(shape, "full", top)) or shape[1:] == (1, 1)
            if shape[1] * shape[2] > 1:
                assert ranges["full"].tolist() == [[1, top]] * shape[0]
                assert ranges["top2"].tolist() == [[top - 1, top]] * shape[0]
                c = S.case(shape, "tails", top).reshape(shape[0], -1)
                assert (c[:, 0] == ranges["tails"][:, 1]).all() and (c[:, -1] == ranges["tails"][:, 0]).all()
            if shape[0] > 1 and shape[1] * shape[2] > 40:
                assert len({tuple(r) for r in ranges["random"].tolist()}) == shape[0]      # a different range per image
            c = S.case(shape, "random", top)
            assert c.dtype == dtype and (shape[1] * shape[2] < 40 or 0.1 < (c == 0).mean() < 0.5)


# ---- the C entries ----------------------------------------------------------------------------------------------------------------

def test_refusals_without_gpu():
    lib = L.load()
    fake, other, third = 4096, 1 << 20, 1 << 21                           # never dereferenced: every call is refused on the host

    def call(entry, B=1, h=5, w=7, src=fake, bits=16, top=65535, lo_hi=third, out=other):
        src = fake + 1 if src == "odd" else src
        lo_hi = third + 2 if lo_hi == "odd" else lo_hi
        p = lambda v: None if v is None else C.c_void_p(v)               # noqa: E731
        if entry == "code_range":
            st = lib.codon_code_range(B, h, w, p(src), bits, p(lo_hi), None)
        else:
            st = getattr(lib, "codon_" + entry)(B, h, w, p(src), bits, top, p(lo_hi), p(out), None)
        return st, lib.codon_last_error_string().decode()

    for entry in ("code_range", "stretch_codes", "unstretch_codes"):
        for kw, word in S.REFUSALS:
            if entry == "code_range" and ("top" in kw or "out" in kw):
                continue
            st, msg = call(entry, **kw)
            assert st == -1 and msg.startswith(entry + ": ") and word in msg, (entry, kw, msg)
    assert call("stretch_codes", out=other + 1)[1] == "stretch_codes: unaligned plane or range"


# ---- the command lines and the Python refusals -------------------------------------------------------------------------------------

def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_cli_refusals_and_defaults(capsys):
    with pytest.raises(SystemExit):
        infer.main(["--input-depth", "d", "--input-color", "c", "--normalize"])
    err = capsys.readouterr().err
    assert "--normalize needs --lr-depth" in err and "--input-depth" in err
    with pytest.raises(SystemExit):
        train.parse_args(_argv("--normalize", "--train-label", "l"))
    assert "--normalize and --train-label exclude each other" in capsys.readouterr().err
    a = train.parse_args(_argv())
    assert a.normalize is False and "normalize" not in train.run_args(a)
    assert train.NORM_DEFAULTS == {"normalize": False}
    for extra in ((), ("--degrade-holes",), ("--train-lr-depth", "l"), ("--train-lr-depth", "l", "--fill-holes")):
        a = train.parse_args(_argv("--normalize", *extra))
        assert a.normalize is True and train.run_args(a)["normalize"] is True
        assert "normalize" not in train.run_args(train.parse_args(_argv(*extra)))
    with pytest.raises(ValueError, match="run_loop: normalize needs lr_depth"):
        infer.run_loop(None, None, torch.float32, "d", "c", normalize=True)
    with pytest.raises(ValueError, match="depth_max 1 leaves per-image normalisation no grid"):
        infer.run_loop(None, None, torch.float32, None, "c", lr_depth="d", scale=4, files=[], depth_bits=16, depth_max=1,
                       normalize=True)


def _write_set(root):
    g = np.random.default_rng(1)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "label")]
    for d in dirs:
        os.makedirs(d)
    for d in dirs:
        io.write_gray(os.path.join(d, "00.png"), g.integers(1, 256, size=(40, 48)).astype(np.uint8))
    return dirs


def test_python_refusals(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path))
    with pytest.raises(ValueError, match="TrainSet: normalize and label_dir exclude each other"):
        train.TrainSet(dd, cd, "cpu", label_dir=ld, normalize=True)
    with pytest.raises(ValueError, match="TrainSet: normalize: depth_max 1 leaves"):
        train.TrainSet(dd, cd, "cpu", depth_bits=16, depth_max=1, normalize=True)
    ts = train.TrainSet(dd, cd, "cpu")
    assert ts.normalize is False
    with pytest.raises(ValueError, match="fit: normalize True with a TrainSet built with normalize False"):
        train.fit(None, ts, 1, scale=4, crop=32, batch=1, normalize=True)
    ts.prep = dataclasses.replace(ts.prep, normalize=True)                # as one built with the option says
    with pytest.raises(ValueError, match="fit: normalize False with a TrainSet built with normalize True"):
        train.fit(None, ts, 1, scale=4, crop=32, batch=1)
    from codon_amd.upsample import code_range, stretch_codes, unstretch_codes
    lo_hi = torch.zeros(1, 2, dtype=torch.int32)
    for bad in (torch.zeros(3, dtype=torch.uint8), torch.zeros(2, 3, 4, 5, dtype=torch.uint8), torch.zeros(4, 5, dtype=torch.int32),
                torch.zeros(4, 5), torch.zeros(1, 1, 4, 5)):
        with pytest.raises(RuntimeError, match="code_range expects"):
            code_range(bad)
        with pytest.raises(RuntimeError, match="unstretch_codes expects"):
            unstretch_codes(bad, lo_hi)
        with pytest.raises(RuntimeError, match="stretch_codes expects"):
            stretch_codes(bad)
    with pytest.raises(ValueError, match="depth_max 1000 with 8-bit codes"):
        stretch_codes(torch.zeros(4, 5, dtype=torch.uint8), depth_max=1000)
    with pytest.raises(ValueError, match="stretch_codes: depth_max 1 leaves"):
        stretch_codes(torch.zeros(4, 5, dtype=torch.int16), depth_max=1)
    with pytest.raises(ValueError, match="unstretch_codes: depth_max 1 leaves"):
        unstretch_codes(torch.zeros(4, 5, dtype=torch.int16), lo_hi, depth_max=1)
    with pytest.raises(ValueError, match="an empty map"):
        code_range(torch.zeros(0, 5, dtype=torch.uint8))
    with pytest.raises(ValueError, match="lo_hi is needed"):
        unstretch_codes(torch.zeros(4, 5, dtype=torch.uint8), None)


def test_resume_of_a_checkpoint_without_the_key(tmp_path):
    """A checkpoint written before the option existed resumes under the defaults, and is refused by name with the option."""
    args = train.run_args(train.parse_args(_argv()))
    assert "normalize" not in args
    path = str(tmp_path / "old.pth")
    torch.save({"epoch": 2, "model": {}, "optimizer": {}, "rng": {}, "args": dict(args)}, path)
    assert train.load_resume(path, args)["epoch"] == 2
    with pytest.raises(ValueError, match="normalize False != True"):
        train.load_resume(path, train.run_args(train.parse_args(_argv("--normalize"))))
    norm = dict(args, normalize=True)
    torch.save({"epoch": 2, "model": {}, "optimizer": {}, "rng": {}, "args": norm}, path)
    assert train.load_resume(path, norm)["epoch"] == 2
    with pytest.raises(ValueError, match="normalize True != False"):
        train.load_resume(path, args)
