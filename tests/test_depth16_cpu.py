"""CPU checks of the 16-bit depth path: the PNG plumbing, TrainSet's refusals and pool layout against the numpy
restatement (tests/train_data16_ref.py), the tables, the restatement's own rounding against float64, the host-side refusals
of the four new ABI entries, and that the 8-bit defaults keep the command line, the checkpoint keys and the pool they had.
No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import io, train
from tests import train_data16_ref as R16
from tests import train_data_ref as R

EDGE = np.array([[0, 1, 255, 256, 65535], [65535, 256, 255, 1, 0], [3, 5003, 10003, 20003, 40003]], dtype=np.uint16)


_write16 = R16.write_set


# ---- PNG plumbing ----------------------------------------------------------------------------------------------------------------

def test_read_depth_and_write_depth16_round_trip(tmp_path):
    from PIL import Image
    p = str(tmp_path / "e.png")
    io.write_depth16(p, EDGE)
    assert Image.open(p).mode in io.DEPTH16_MODES
    got = io.read_depth(p)
    assert got.dtype == np.uint16 and np.array_equal(got, EDGE)
    # read_gray is untouched: on a 16-bit file it still clips at 255, as it always did
    assert np.array_equal(io.read_gray(p), np.minimum(EDGE, 255).astype(np.uint8))
    q = str(tmp_path / "g.png")
    g8 = np.arange(12, dtype=np.uint8).reshape(3, 4) * 23
    io.write_gray(q, g8)
    assert io.read_depth(q).dtype == np.uint8 and np.array_equal(io.read_depth(q), io.read_gray(q))
    r = str(tmp_path / "i.tif")                                   # mode I: 32-bit integers
    Image.fromarray(EDGE.astype(np.int32)).save(r)
    assert Image.open(r).mode == "I" and np.array_equal(io.read_depth(r), EDGE)
    big = str(tmp_path / "big.tif")
    Image.fromarray(np.array([[0, 65536]], dtype=np.int32)).save(big)
    assert Image.open(big).mode == "I"
    with pytest.raises(ValueError, match="big.tif"):
        io.read_depth(big)


# ---- TrainSet: refusals and layout -----------------------------------------------------------------------------------------------

def test_trainset_refusals_name_the_file(tmp_path):
    dd, cd, ld, _ = _write16(str(tmp_path), [(20, 24), (21, 23)], depth_max=10000)
    with pytest.raises(ValueError, match=r"00\.png.*--depth-bits 16"):              # used to pass, saturated at 255
        train.TrainSet(dd, cd, "cpu")
    with pytest.raises(ValueError, match=r"label.00\.png.*--depth-bits 16"):        # an 8-bit depth with a 16-bit label
        train.TrainSet(cd, cd, "cpu", label_dir=ld)
    with pytest.raises(ValueError, match=r"color.00\.png.*8-bit image in a 16-bit"):
        train.TrainSet(cd, cd, "cpu", depth_bits=16)
    with pytest.raises(ValueError, match=r"color.00\.png.*8-bit image in a 16-bit"):
        train.TrainSet(dd, cd, "cpu", label_dir=cd, depth_bits=16, depth_max=10000)
    with pytest.raises(ValueError, match=r"00\.png: code 10000 lies above depth_max 9999"):
        train.TrainSet(dd, cd, "cpu", depth_bits=16, depth_max=9999)
    os.remove(os.path.join(ld, "01.png"))
    with pytest.raises(ValueError, match=r"01\.png has no namesake"):
        train.TrainSet(dd, cd, "cpu", label_dir=ld, depth_bits=16, depth_max=10000)
    for bad in (0, 65536, 1.5):
        with pytest.raises(ValueError, match="depth_max"):
            train.TrainSet(dd, cd, "cpu", depth_bits=16, depth_max=bad)
    with pytest.raises(ValueError, match="depth_bits"):
        train.TrainSet(dd, cd, "cpu", depth_bits=12)


@pytest.mark.parametrize("label", [False, True])
def test_pool16_equals_the_restatement(tmp_path, label):
    sizes = [(37, 53), (40, 64), (37, 53)]                         # odd H*W: one byte of padding after the record
    dd, cd, ld, planes = _write16(str(tmp_path), sizes, label=label)
    ts = train.TrainSet(dd, cd, "cpu", label_dir=ld, depth_bits=16)
    want, offsets = R16.pack(planes)
    assert ts.pool.dtype == torch.uint8 and np.array_equal(ts.pool.numpy(), want)
    assert ts.offsets.tolist() == offsets and all(o % 2 == 0 for o in offsets)
    per = 5 if label else 3
    assert offsets[1] == per * 37 * 53 + 1 and offsets[2] == offsets[1] + per * 40 * 64
    assert ts.sizes.tolist() == [list(s) for s in sizes] and (ts.depth_bits, ts.depth_max) == (16, 65535)
    for off, (h, w), (dep, lab, gui) in zip(offsets, sizes, planes):
        d, l, g = R16.planes(want, off, h, w, label)
        assert np.array_equal(d, dep) and np.array_equal(g, gui) and (lab is None or np.array_equal(l, lab))
    # the integral images see the u16 target plane: the label if there is one, else the depth map
    ii = ts.valid_integrals()
    for off, (dep, lab, _) in zip(offsets, planes):
        tgt = lab if label else dep
        assert int(ii[off][-1, -1]) == int((tgt != 0).sum()) and int(ii[off][5, 7]) == int((tgt[:5, :7] != 0).sum())
    descs = train.draw(np.random.default_rng(1), ts, 8, 16, min_valid=0.5)
    assert set(descs[:, 0].tolist()) <= set(offsets)


def test_pool8_is_what_it_was(tmp_path):
    g = np.random.default_rng(3)
    dd, cd = str(tmp_path / "d"), str(tmp_path / "c")
    os.makedirs(dd)
    os.makedirs(cd)
    a, b = g.integers(0, 256, (37, 53), dtype=np.uint8), g.integers(0, 256, (38, 53), dtype=np.uint8)
    io.write_gray(os.path.join(dd, "0.png"), a)
    io.write_gray(os.path.join(cd, "0.png"), b)
    ts = train.TrainSet(dd, cd, "cpu")
    assert np.array_equal(ts.pool.numpy(), np.concatenate([a.reshape(-1), b[:37].reshape(-1)])) and ts.offsets.tolist() == [0]
    assert (ts.depth_bits, ts.depth_max) == (8, 65535)


# ---- tables and the restatement's own arithmetic -----------------------------------------------------------------------------------

def test_lut16_ties_to_u8_lut():
    t16, t8 = train.lut16(65535), train.u8_lut()
    assert t16.dtype == np.float32 and t16.shape == (65536,)
    assert np.array_equal(t16[257 * np.arange(256)].view(np.uint32), t8.view(np.uint32))
    for m in (65535, 10000, 4096, 1):
        assert np.array_equal(train.lut16(m).view(np.uint32), R16.lut16(m).view(np.uint32))
        assert train.lut16(m)[0] == 0.0 and train.lut16(m)[m] == 1.0
    for bad in (0, 65536):
        with pytest.raises(ValueError):
            train.lut16(bad)


def test_restatement_rounding_against_float64():
    g = np.random.default_rng(0)
    for m in (65535, 10000, 4096):
        x = g.uniform(-0.1, 1.1, 20000).astype(np.float32)
        exact = np.clip(x.astype(np.float64), 0, 1) * m              # float64: exact product of a float32 and an integer
        frac = np.abs(exact - np.floor(exact) - 0.5)
        # the fp32 product is off by at most half an ulp of a value below 2^16, 2^-9: farther than 2^-8 from a tie it rounds
        # to the integer the exact product rounds to
        keep = frac > 2.0 ** -8
        codes = np.rint(exact).astype(np.int64)
        assert keep.sum() > 19000
        assert np.array_equal(R16.quantize(x, m)[keep], R16.lut16(m)[codes[keep]])
        assert np.array_equal(R16.postprocess_u16(x, m)[keep], codes[keep].astype(np.uint16))
    k = np.arange(0, 4096)
    ties = ((k + 0.5) / 4096).astype(np.float32)                     # exact in fp32, and so is the product k + 0.5
    assert np.array_equal(ties.astype(np.float64) * 4096, k + 0.5)
    even = (k + (k % 2)).astype(np.uint16)                           # half to even
    assert np.array_equal(R16.postprocess_u16(ties, 4096), even)
    assert np.array_equal(R16.quantize(ties, 4096), R16.lut16(4096)[even])
    sp = np.array([np.nan, -1.0, -0.0, 0.0, 2.0, np.inf, -np.inf], dtype=np.float32)
    assert R16.postprocess_u16(sp, 10000).tolist() == [0, 0, 0, 0, 10000, 10000, 0]
    assert R16.postprocess_u16(np.array([0.5, 1.0], dtype=np.float16), 65535).tolist() == [32768, 65535]
    assert R16.postprocess_u16(np.array([0x3F00, 0x3F80, 0x7FC0], dtype=np.uint16), 65535).tolist() == [32768, 65535, 0]   # bf16 bits
    lab = np.array([[0, 65535, 1], [7, 0, 0]], dtype=np.uint16)
    out = np.array([[9, 0, 65535], [7, 1, 2]], dtype=np.uint16)
    assert R16.masked_sqerr(lab, out) == (65535 ** 2 + 65534 ** 2, 3)


def test_restatement_crops_and_d4():
    g = np.random.default_rng(5)
    dep = g.integers(0, 65536, (9, 11)).astype(np.uint16)
    lab = g.integers(0, 65536, (9, 11)).astype(np.uint16)
    gui = g.integers(0, 256, (9, 11), dtype=np.uint8)
    pool, offs = R16.pack([(dep, lab, gui), (dep, lab, gui)])
    assert offs == [0, 5 * 99 + 1]
    for op in range(8):
        s, y, t = R16.crops(pool, [[offs[1], 9, 11, 2, 3, op]], 5, 65535, True)
        assert np.array_equal(s[0, 0], R16.lut16()[R.d4(dep[2:7, 3:8], op)])
        assert np.array_equal(t[0, 0], R16.lut16()[R.d4(lab[2:7, 3:8], op)])
        assert np.array_equal(y[0, 0], R.lut()[R.d4(gui[2:7, 3:8], op)])
    pool2, _ = R16.pack([(dep, None, gui)])
    s, y, t = R16.crops(pool2, [[0, 9, 11, 0, 0, 3]], 9, 4096, False)
    assert t is not None and np.array_equal(s, t) and np.array_equal(y[0, 0], R.lut()[R.d4(gui[:9, :9], 3)])


# ---- the ABI's refusals, on the host ---------------------------------------------------------------------------------------------

def test_native_refusals_without_gpu():
    from codon_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(256)                    # never dereferenced: every call below is refused on the host

    def crops(rows, crop=32, pool_bytes=1 << 20, n=None, lut16=fake, lut8=fake, source=fake, guide=fake, target=fake, pool=fake):
        d = L.CropDesc()
        d.n, d.crop = len(rows) if n is None else n, crop
        for b, (off, h, w, y0, x0, op) in enumerate(rows):
            s = d.s[b]
            s.offset, s.height, s.width, s.y0, s.x0, s.op = off, h, w, y0, x0, op
        st = lib.codon_train_crops_u16(C.byref(d), pool, pool_bytes, lut16, lut8, source, guide, target, None)
        return st, lib.codon_last_error_string().decode()

    ok = (0, 40, 48, 8, 16, 7)
    for kw in ({"lut16": None}, {"lut8": None}, {"source": None}, {"guide": None}, {"pool": None}):
        assert crops([ok], **kw) == (-1, "train_crops_u16: null pointer")
    assert crops([ok, (0, 40, 48, 9, 0, 0)])[1].startswith("train_crops_u16: sample 1: 40x48 crop at (9, 0) op 0 outside the image")
    assert crops([(0, 40, 48, 0, 17, 0)])[0] == -1 and crops([(0, 40, 48, -1, 0, 0)])[0] == -1
    assert crops([(0, 40, 48, 0, 0, 8)])[0] == -1
    st, msg = crops([ok, (1, 40, 48, 0, 0, 0)])
    assert st == -1 and "sample 1" in msg and "odd" in msg
    assert "odd" in crops([(-2, 40, 48, 0, 0, 0)])[1]
    assert "past the" in crops([ok], pool_bytes=5 * 40 * 48 - 1)[1]                  # labeled: 5 bytes per pixel
    assert "past the" in crops([ok], pool_bytes=3 * 40 * 48 - 1, target=None)[1]     # unlabeled: 3
    assert crops([ok], pool_bytes=5 * 40 * 48 - 1)[0] == -1 and crops([ok], pool_bytes=3 * 40 * 48 - 1, target=None)[0] == -1
    odd = (0, 33, 35, 0, 0, 0)                # records of odd size: the pad byte is not the record's, one byte short is refused
    assert crops([odd], pool_bytes=5 * 33 * 35 - 1)[0] == -1 and "past the 5774-byte" in crops([odd], pool_bytes=5 * 33 * 35 - 1)[1]
    assert crops([odd], pool_bytes=3 * 33 * 35 - 1, target=None)[0] == -1
    assert "past the" in crops([((1 << 33), 40, 48, 0, 0, 0)], pool_bytes=(1 << 33) + 5 * 40 * 48 - 2)[1]
    assert "batch 65" in crops([ok], n=L.TRAIN_MAX_BATCH + 1)[1]
    assert "batch 0" in crops([], n=0)[1]

    def err(st):
        return st, lib.codon_last_error_string().decode()

    assert err(lib.codon_quantize_levels(0, fake, fake, 4096, None))[0] == -1
    assert err(lib.codon_quantize_levels(8, None, fake, 4096, None))[0] == -1
    assert err(lib.codon_quantize_levels(8, fake, None, 4096, None))[0] == -1
    assert "depth_max 0 " in err(lib.codon_quantize_levels(8, fake, fake, 0, None))[1]
    assert "depth_max 65536 " in err(lib.codon_quantize_levels(8, fake, fake, 65536, None))[1]
    assert err(lib.codon_postprocess_u16_dt(8, None, L.F32, 4096, fake, None))[0] == -1
    assert err(lib.codon_postprocess_u16_dt(8, fake, L.F32, 4096, None, None))[0] == -1
    assert err(lib.codon_postprocess_u16_dt(0, fake, L.F32, 4096, fake, None))[0] == -1
    assert err(lib.codon_postprocess_u16_dt(8, fake, 3, 4096, fake, None))[0] == -2
    assert "depth_max 0 " in err(lib.codon_postprocess_u16_dt(8, fake, L.F16, 0, fake, None))[1]
    assert "depth_max 65536 " in err(lib.codon_postprocess_u16_dt(8, fake, L.BF16, 65536, fake, None))[1]
    for args in ((8, None, fake, fake), (8, fake, None, fake), (8, fake, fake, None), (0, fake, fake, fake)):
        assert err(lib.codon_masked_sqerr_u16(*args, None))[0] == -1
    assert "2^26" in err(lib.codon_masked_sqerr_u16((1 << 26) + 1, fake, fake, fake, None))[1]
    assert lib.codon_abi_version() == 1


# ---- the command lines and the checkpoint keys -------------------------------------------------------------------------------------

PARENT_ARG_KEYS = {"scale", "crop", "batch", "dtype", "lr", "seed", "clip_norm", "skip_nonfinite", "ema", "lr_schedule",
                   "warmup_steps", "lr_min", "lr_steps", "mask_holes", "min_valid", "train_label"}


def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_train_cli_and_resume_keys(tmp_path, capsys):
    a = train.parse_args(_argv())
    assert (a.depth_bits, a.depth_max) == (8, 65535)
    assert set(train.run_args(a)) == PARENT_ARG_KEYS                       # 8-bit: exactly the keys checkpoints always had
    b = train.parse_args(_argv("--depth-bits", "16", "--depth-max", "10000"))
    args16 = train.run_args(b)
    assert set(args16) == PARENT_ARG_KEYS | {"depth_bits", "depth_max"} and (args16["depth_bits"], args16["depth_max"]) == (16, 10000)
    assert train.run_args(train.parse_args(_argv("--depth-bits", "16")))["depth_max"] == 65535
    for bad in (["--depth-max", "10000"], ["--depth-bits", "16", "--depth-max", "0"], ["--depth-bits", "16", "--depth-max", "65536"],
                ["--depth-bits", "12"]):
        with pytest.raises(SystemExit):
            train.parse_args(_argv(*bad))
    capsys.readouterr()
    assert train.DEPTH_DEFAULTS == {"depth_bits": 8, "depth_max": 65535}
    ck = {"epoch": 2, "model": {}, "optimizer": {}, "rng": np.random.default_rng(0).bit_generator.state}
    p = str(tmp_path / "ck.pth")
    torch.save(dict(ck, args=train.run_args(a)), p)                        # an 8-bit checkpoint: no depth keys at all
    assert train.load_resume(p, train.run_args(a))["epoch"] == 2
    with pytest.raises(ValueError, match="other arguments: depth_bits 8 != 16"):
        train.load_resume(p, args16)
    torch.save(dict(ck, args=args16), p)
    assert train.load_resume(p, args16)["epoch"] == 2
    with pytest.raises(ValueError, match="depth_max 10000 != 4096"):
        train.load_resume(p, dict(args16, depth_max=4096))
    with pytest.raises(ValueError, match="depth_bits 16 != 8"):
        train.main(_argv("--resume", p))                                   # refused before any device or file work


def test_infer_load_host(tmp_path):
    from codon_amd import infer
    dd, cd, ld, planes = _write16(str(tmp_path), [(20, 24)], depth_max=10000)
    x, y, lab, h, w = infer._load_host(dd, cd, ld, "00.png", torch.float32, 16, 10000)
    dep, label, gui = planes[0]
    assert (h, w) == (20, 24) and x.dtype == torch.float32
    assert np.array_equal(x[0, 0].numpy(), R16.lut16(10000)[dep]) and np.array_equal(y[0, 0].numpy(), R.lut()[gui])
    assert lab.dtype == torch.int16 and np.array_equal(lab.numpy().view(np.uint16), label)
    xh = infer._load_host(dd, cd, None, "00.png", torch.float16, 16, 10000)[0]
    assert np.array_equal(xh[0, 0].numpy(), R16.lut16(10000)[dep].astype(np.float16))
    with pytest.raises(ValueError, match=r"00\.png.*--depth-bits 16"):
        infer._load_host(dd, cd, None, "00.png", torch.float32)
    with pytest.raises(ValueError, match=r"label.00\.png.*--depth-bits 16"):
        infer._load_host(cd, cd, ld, "00.png", torch.float32)
    with pytest.raises(ValueError, match="above depth_max 4096"):
        infer._load_host(dd, cd, None, "00.png", torch.float32, 16, 4096)
    x8, y8, lab8, _, _ = infer._load_host(cd, cd, cd, "00.png", torch.float32)
    g = io.read_gray(os.path.join(cd, "00.png"))
    assert np.array_equal(x8[0, 0].numpy(), io.to_input(g)[0, 0].numpy()) and lab8.dtype == torch.uint8
