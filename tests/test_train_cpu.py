"""CPU checks of codon_amd.train: the numpy definition of the degradation (tests/train_data_ref.py) against torch's
antialiased bicubic and numpy's D4 identities, the host tables of the product against it, the batch drawing and sharding,
and the command line's refusals.  No GPU."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from codon_amd import io, train
from tests import train_data_ref as R


def _write_set(root, sizes, seed=0):
    rng = np.random.default_rng(seed)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd)
    os.makedirs(cd)
    for i, (h, w) in enumerate(sizes):
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), rng.integers(0, 256, size=(h, w), dtype=np.uint8))
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), rng.integers(0, 256, size=(h + i, w + 1), dtype=np.uint8))
    return dd, cd


@pytest.mark.parametrize("s", [4, 8, 16])
def test_downsample_definition_matches_torch_antialias(s):
    rng = np.random.default_rng(s)
    for P in (4 * s, 6 * s, 128):
        x = rng.random((2, 1, P, P)).astype(np.float32)
        x[0, 0, 0, :] = 1.0                    # strong edges on the borders: the renormalised taps matter there
        x[1, 0, :, -1] = 0.0
        ref = F.interpolate(torch.from_numpy(x).double(), scale_factor=1 / s, mode="bicubic", antialias=True,
                            align_corners=False).numpy()
        got = R.downsample(x, s)
        assert got.shape == ref.shape == (2, 1, P // s, P // s)
        assert float(np.abs(got - ref).max()) <= 1e-6


def test_product_tables_equal_the_definition():
    for s in (4, 8, 16):
        for P in (4 * s, 5 * s, 128, 256):
            assert np.array_equal(train.down_weights(P, s), R.down_weights(P, s)), (s, P)
    codes = np.arange(256, dtype=np.uint8).reshape(16, 16)
    assert np.array_equal(train.u8_lut()[codes][None, None], io.to_input(codes).numpy())
    assert np.array_equal(R.lut(), train.u8_lut())


def test_d4_codes_are_the_eight_symmetries():
    c = np.arange(25).reshape(5, 5)
    want = {0: c, 1: c.T, 2: np.flipud(c), 3: np.rot90(c, 1), 4: np.fliplr(c), 5: np.rot90(c, -1), 6: np.rot90(c, 2),
            7: np.rot90(c, 2).T}
    for op in range(8):
        assert np.array_equal(R.d4(c, op), want[op]), op
    assert len({R.d4(c, op).tobytes() for op in range(8)}) == 8


def test_quantize_definition():
    x = np.array([-1.0, 0.0, 0.5 / 255, 1.5 / 255, 2.5 / 255, 0.5, 1.0, 7.0], dtype=np.float32)
    q = R.quantize(x)
    codes = np.rint(np.clip(x, 0, 1) * np.float32(255)).astype(int)
    assert np.array_equal(q, R.lut()[codes])
    assert np.array_equal(R.quantize(q), q)                                # idempotent on 8-bit values


def test_trainset_and_draw(tmp_path):
    dd, cd = _write_set(str(tmp_path), [(40, 48), (36, 50), (64, 33)])
    ts = train.TrainSet(dd, cd, "cpu")
    assert len(ts) == 3 and ts.sizes.tolist() == [[40, 48], [36, 50], [64, 33]]
    assert ts.offsets.tolist() == [0, 2 * 40 * 48, 2 * (40 * 48 + 36 * 50)]
    pool = ts.pool.numpy()
    assert np.array_equal(pool[:40 * 48].reshape(40, 48), io.read_gray(os.path.join(dd, "00.png")))
    assert np.array_equal(pool[40 * 48:2 * 40 * 48].reshape(40, 48), io.read_gray(os.path.join(cd, "00.png"))[:40, :48])

    a = train.draw(np.random.default_rng(7), ts, 8, 32)
    b = train.draw(np.random.default_rng(7), ts, 8, 32)
    assert a.shape == (8, 6) and a.dtype == np.int64 and np.array_equal(a, b)
    assert (a[:, 3] + 32 <= a[:, 1]).all() and (a[:, 4] + 32 <= a[:, 2]).all() and (a[:, 3:5] >= 0).all()
    assert set(a[:, 5].tolist()) <= set(range(8))
    for world in (1, 2, 4):
        parts = [train.draw(np.random.default_rng(7), ts, 8, 32, r, world) for r in range(world)]
        assert np.array_equal(np.concatenate(parts), a)
    with pytest.raises(ValueError, match="split evenly"):
        train.draw(np.random.default_rng(0), ts, 6, 32, 0, 4)
    with pytest.raises(ValueError, match="does not fit"):
        train.draw(np.random.default_rng(0), ts, 4, 34)
    with pytest.raises(ValueError, match="smaller than"):
        train.TrainSet(dd, cd, "cpu", crop=34)


def test_draw_generator_stays_in_step_across_ranks(tmp_path):
    """Every rank consumes the same draws, so the generators of all ranks hold the same state after every step."""
    dd, cd = _write_set(str(tmp_path), [(40, 48), (36, 50)])
    ts = train.TrainSet(dd, cd, "cpu")
    gens = [np.random.default_rng(3) for _ in range(4)]
    for _ in range(3):
        for r, g in enumerate(gens):
            train.draw(g, ts, 8, 16, r, 4)
    assert all(g.bit_generator.state == gens[0].bit_generator.state for g in gens)


def _argv(tmp_path, *extra):
    return ["--scale", "4", "--train-depth", str(tmp_path / "nope_d"), "--train-color", str(tmp_path / "nope_c"), *extra]


def test_cli_refusals(tmp_path, capsys):
    with pytest.raises(SystemExit):
        train.parse_args(_argv(tmp_path, "--crop", "130"))
    assert "multiple of --scale" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        train.parse_args(_argv(tmp_path, "--crop", "12"))
    with pytest.raises(SystemExit):
        train.parse_args(["--scale", "16", "--train-depth", "d", "--train-color", "c", "--crop", "48"])
    with pytest.raises(SystemExit):
        train.parse_args(_argv(tmp_path, "--dtype", "f16"))
    assert "fp16 training" in capsys.readouterr().err
    a = train.parse_args(_argv(tmp_path))
    assert (a.crop, a.batch, a.lr, a.dtype, a.seed) == (128, 16, 1e-4, "bf16", 0)


@pytest.mark.parametrize("field,value", [("scale", 8), ("crop", 64), ("batch", 8), ("dtype", "f32")])
def test_resume_refuses_other_arguments(tmp_path, field, value):
    a = train.parse_args(_argv(tmp_path))
    args = train.run_args(a)
    ck = {"epoch": 2, "model": {}, "optimizer": {}, "rng": np.random.default_rng(0).bit_generator.state,
          "args": dict(args, **{field: value})}
    p = str(tmp_path / "ck.pth")
    torch.save(ck, p)
    with pytest.raises(ValueError, match=f"other arguments: {field}"):
        train.main(_argv(tmp_path, "--resume", p))          # refused before any device or file work
    torch.save(dict(ck, args=args), p)
    assert train.load_resume(p, args)["epoch"] == 2
    torch.save({"model": {}}, p)
    with pytest.raises(ValueError, match="not a codon_amd.train checkpoint"):
        train.load_resume(p, args)


def test_native_refusals_without_gpu():
    """The three entry points validate every descriptor before anything is launched: no window outside its image, no image
    outside the pool, no batch above CODON_TRAIN_MAX_BATCH."""
    import ctypes as C
    from codon_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(256)                    # never dereferenced: every call below is refused on the host

    def crops(rows, crop=32, pool_bytes=1 << 20, n=None):
        d = L.CropDesc()
        d.n, d.crop = len(rows) if n is None else n, crop
        for b, (off, h, w, y0, x0, op) in enumerate(rows):
            s = d.s[b]
            s.offset, s.height, s.width, s.y0, s.x0, s.op = off, h, w, y0, x0, op
        st = lib.codon_train_crops(C.byref(d), fake, pool_bytes, fake, fake, fake, None)
        return st, lib.codon_last_error_string().decode()

    ok = (0, 40, 48, 8, 16, 7)
    assert crops([ok, (0, 40, 48, 9, 0, 0)])[1].startswith("train_crops: sample 1")
    assert crops([(0, 40, 48, 0, 17, 0)])[0] == -1
    assert crops([(0, 40, 48, -1, 0, 0)])[0] == -1
    assert crops([(0, 40, 48, 0, 0, 8)])[0] == -1
    assert "past the" in crops([ok], pool_bytes=2 * 40 * 48 - 1)[1]
    assert crops([ok], pool_bytes=2 * 40 * 48 - 1)[0] == -1                  # the record one byte short: CODON_ERR_BAD_ARG
    assert crops([(0, 33, 35, 0, 0, 0)], pool_bytes=2 * 33 * 35 - 1)[0] == -1
    assert "past the" in crops([((1 << 33), 40, 48, 0, 0, 0)], pool_bytes=(1 << 33) + 2 * 40 * 48 - 1)[1]
    assert "batch 65" in crops([ok], n=L.TRAIN_MAX_BATCH + 1)[1]
    assert "batch 0" in crops([], n=0)[1]
    assert lib.codon_bicubic_downsample(2, 60, 16, fake, fake, fake, None) == -1          # 60 / 16 < 4
    assert lib.codon_bicubic_downsample(2, 66, 4, fake, fake, fake, None) == -1           # not a multiple of the scale
    assert lib.codon_bicubic_downsample(2, 64, 2, fake, fake, fake, None) == -2
    assert lib.codon_quantize_u8(0, fake, fake, None) == -1
