"""CPU checks of the label plane and of hole-aware drawing in codon_amd.train: the three-plane pool, the refusal of a pair
without a label, the integral images, draw(min_valid=) -- deterministic, every crop over the threshold by brute force,
min_valid = 0 exactly today's rows and generator state, an unsatisfiable threshold refused -- the command line's refusals and
the resume keys.  No GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import io, train


def _write_set(root, sizes, seed=0, label=True, holes=0.3):
    """Filled depth maps (no zeros), guidance, and labels = the depth map with holes: isolated zeros and zero blobs."""
    rng = np.random.default_rng(seed)
    dd, cd, ld = (os.path.join(root, n) for n in ("depth", "color", "label"))
    for d in (dd, cd, ld):
        os.makedirs(d, exist_ok=True)
    for i, (h, w) in enumerate(sizes):
        d = rng.integers(1, 256, size=(h, w), dtype=np.uint8)
        lab = d.copy()
        lab[rng.random((h, w)) < 0.02] = 0
        lab[: int(h * holes), : w // 2] = 0                               # a blob: the upper left is mostly hole
        io.write_gray(os.path.join(dd, f"{i:02d}.png"), d)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), rng.integers(0, 256, size=(h + i, w + 1), dtype=np.uint8))
        if label:
            io.write_gray(os.path.join(ld, f"{i:02d}.png"), lab[: h - (i % 2), :])      # a label one row short: common size
    return dd, cd, ld


def test_trainset_label_plane_layout_and_refusal(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path), [(40, 48), (37, 50), (64, 33)])
    ts = train.TrainSet(dd, cd, "cpu", label_dir=ld)
    assert ts.has_label and len(ts) == 3 and ts.sizes.tolist() == [[40, 48], [36, 50], [64, 33]]
    assert ts.offsets.tolist() == [0, 3 * 40 * 48, 3 * (40 * 48 + 36 * 50)]
    pool = ts.pool.numpy()
    assert pool.size == 3 * (40 * 48 + 36 * 50 + 64 * 33)
    off, (h, w) = int(ts.offsets[1]), (36, 50)
    for k, d in enumerate((dd, cd, ld)):
        assert np.array_equal(pool[off + k * h * w:off + (k + 1) * h * w].reshape(h, w), io.read_gray(os.path.join(d, "01.png"))[:h, :w])
    os.remove(os.path.join(ld, "02.png"))
    with pytest.raises(ValueError, match="02.png has no namesake"):
        train.TrainSet(dd, cd, "cpu", label_dir=ld)
    # without a label directory nothing changes: two planes, today's offsets
    ts2 = train.TrainSet(dd, cd, "cpu")
    assert not ts2.has_label and ts2.offsets.tolist() == [0, 2 * 40 * 48, 2 * (40 * 48 + 37 * 50)]


def test_integral_images_count_the_target_plane(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path), [(40, 48), (36, 50)])
    ts = train.TrainSet(dd, cd, "cpu", label_dir=ld)
    ii = ts.valid_integrals()
    for i, f in enumerate(ts.files):
        h, w = ts.sizes[i].tolist()
        lab = io.read_gray(os.path.join(ld, f))[:h, :w]
        t = ii[int(ts.offsets[i])]
        assert t.dtype == np.int32 and t.shape == (h + 1, w + 1) and t[-1, -1] == (lab != 0).sum()
    descs = np.asarray([[int(ts.offsets[1]), 36, 50, 3, 7, 5], [0, 40, 48, 8, 16, 0]])
    lab1 = io.read_gray(os.path.join(ld, "01.png"))[:36, :50]
    lab0 = io.read_gray(os.path.join(ld, "00.png"))[:40, :48]
    want = [(lab1[3:35, 7:39] != 0).sum(), (lab0[8:40, 16:48] != 0).sum()]
    assert train.valid_counts(ts, descs, 32).tolist() == want
    # no label: validity is the depth map's (filled here: every pixel valid)
    ts2 = train.TrainSet(dd, cd, "cpu")
    assert train.valid_counts(ts2, np.asarray([[0, 40, 48, 8, 16, 0]]), 32).tolist() == [32 * 32]


def _brute_valid(ts, row, crop):
    off, h, w, y0, x0, _ = row
    plane = 2 if ts.has_label else 0
    img = ts.pool.numpy()[off + plane * h * w:off + (plane + 1) * h * w].reshape(h, w)
    return int((img[y0:y0 + crop, x0:x0 + crop] != 0).sum())


def test_draw_min_valid(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path), [(60, 64), (56, 70), (64, 53)], holes=0.6)
    ts = train.TrainSet(dd, cd, "cpu", label_dir=ld)
    crop, thr = 24, 0.8
    # min_valid = 0: the rows and the generator state of a call without the option
    g0, g1 = np.random.default_rng(11), np.random.default_rng(11)
    for _ in range(3):
        assert np.array_equal(train.draw(g0, ts, 8, crop), train.draw(g1, ts, 8, crop, min_valid=0.0))
    assert g0.bit_generator.state == g1.bit_generator.state
    # the threshold bites on this set: plain draws fall below it
    plain = np.concatenate([train.draw(np.random.default_rng(s), ts, 16, crop) for s in range(4)])
    assert min(_brute_valid(ts, r, crop) for r in plain.tolist()) < thr * crop * crop
    ga, gb = np.random.default_rng(12), np.random.default_rng(12)
    for _ in range(6):
        a = train.draw(ga, ts, 16, crop, min_valid=thr)
        b = train.draw(gb, ts, 16, crop, min_valid=thr)
        assert np.array_equal(a, b) and a.shape == (16, 6) and a.dtype == np.int64
        for r in a.tolist():
            assert _brute_valid(ts, r, crop) >= thr * crop * crop, r
            assert 0 <= r[3] <= r[1] - crop and 0 <= r[4] <= r[2] - crop and 0 <= r[5] < 8
            i = ts.offsets.tolist().index(r[0])
            assert ts.sizes[i].tolist() == r[1:3]
    assert ga.bit_generator.state == gb.bit_generator.state
    # every rank redraws the whole batch: the shards concatenate to it and the generators stay in step
    gens = [np.random.default_rng(13) for _ in range(2)]
    parts = [train.draw(g, ts, 16, crop, r, 2, min_valid=thr) for r, g in enumerate(gens)]
    assert np.array_equal(np.concatenate(parts), train.draw(np.random.default_rng(13), ts, 16, crop, min_valid=thr))
    assert gens[0].bit_generator.state == gens[1].bit_generator.state
    with pytest.raises(ValueError, match="must lie in"):
        train.draw(np.random.default_rng(0), ts, 4, crop, min_valid=1.5)


def test_draw_min_valid_unsatisfiable_raises(tmp_path):
    dd, cd, ld = _write_set(str(tmp_path), [(40, 48)], holes=0.0)
    ts = train.TrainSet(dd, cd, "cpu", label_dir=ld)
    with pytest.raises(ValueError, match=r"min_valid = 1\.0"):              # 2 % isolated holes: no 32x32 crop is hole-free
        train.draw(np.random.default_rng(0), ts, 4, 32, min_valid=1.0)


def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_cli_options_and_refusals(capsys):
    a = train.parse_args(_argv())
    assert (a.train_label, a.mask_holes, a.min_valid) == (None, False, 0.0)
    r = train.run_args(a)
    assert all(r[k] == train.RESUME_DEFAULTS[k] for k in ("mask_holes", "min_valid", "train_label"))
    a = train.parse_args(_argv("--train-label", "l", "--mask-holes", "--min-valid", "0.25"))
    r = train.run_args(a)
    assert (r["train_label"], r["mask_holes"], r["min_valid"]) == (True, True, 0.25)
    with pytest.raises(SystemExit):
        train.parse_args(_argv("--min-valid", "0.5"))
    assert "--min-valid needs --mask-holes" in capsys.readouterr().err
    for bad in ("-0.1", "1.5"):
        with pytest.raises(SystemExit):
            train.parse_args(_argv("--mask-holes", "--min-valid", bad))
        assert "must lie in [0, 1]" in capsys.readouterr().err


def test_resume_keys_defaults_and_older_checkpoints(tmp_path):
    assert {"mask_holes", "min_valid", "train_label"} <= set(train.RESUME_KEYS)
    assert (train.RESUME_DEFAULTS["mask_holes"], train.RESUME_DEFAULTS["min_valid"], train.RESUME_DEFAULTS["train_label"]) == \
        (False, 0.0, False)
    base = ("scale", "crop", "batch", "dtype")                                # the keys every checkpoint carries
    assert set(train.RESUME_KEYS) == set(base) | set(train.RESUME_DEFAULTS)
    plain = train.run_args(train.parse_args(_argv()))
    old = {k: v for k, v in plain.items() if k not in ("mask_holes", "min_valid", "train_label")}
    ck = {"epoch": 2, "model": {}, "optimizer": {}, "rng": np.random.default_rng(0).bit_generator.state, "args": old}
    p = str(tmp_path / "ck.pth")
    torch.save(ck, p)
    assert train.load_resume(p, plain)["epoch"] == 2                          # a checkpoint without the new keys resumes
    masked = train.run_args(train.parse_args(_argv("--mask-holes", "--min-valid", "0.5", "--train-label", "l")))
    with pytest.raises(ValueError, match="other arguments: mask_holes False != True, min_valid 0.0 != 0.5, train_label False != True"):
        train.load_resume(p, masked)
    torch.save(dict(ck, args=masked), p)
    assert train.load_resume(p, masked)["epoch"] == 2
    with pytest.raises(ValueError, match="mask_holes True != False"):
        train.load_resume(p, plain)


def test_labeled_entry_refusals_without_gpu():
    """codon_train_crops_labeled validates like codon_train_crops, with records of three planes."""
    from codon_amd import _lib as L
    lib = L.load()
    fake = C.c_void_p(256)                    # never dereferenced: every call below is refused on the host

    def crops(rows, crop=32, pool_bytes=1 << 20, n=None):
        d = L.CropDesc()
        d.n, d.crop = len(rows) if n is None else n, crop
        for b, (off, h, w, y0, x0, op) in enumerate(rows):
            s = d.s[b]
            s.offset, s.height, s.width, s.y0, s.x0, s.op = off, h, w, y0, x0, op
        st = lib.codon_train_crops_labeled(C.byref(d), fake, pool_bytes, fake, fake, fake, fake, None)
        return st, lib.codon_last_error_string().decode()

    ok = (0, 40, 48, 8, 16, 7)
    assert crops([ok, (0, 40, 48, 9, 0, 0)])[1].startswith("train_crops_labeled: sample 1")
    assert crops([(0, 40, 48, 0, 0, 8)])[0] == -1
    assert "past the" in crops([ok], pool_bytes=3 * 40 * 48 - 1)[1]          # two planes fit, the label does not
    assert crops([ok], pool_bytes=3 * 40 * 48 - 1)[0] == -1
    assert crops([(0, 33, 35, 0, 0, 0)], pool_bytes=3 * 33 * 35 - 1) == (
        -1, "train_crops_labeled: sample 0: the record at offset 0 runs past the 3464-byte pool")
    assert "batch 65" in crops([ok], n=L.TRAIN_MAX_BATCH + 1)[1]
    d = L.CropDesc()
    assert lib.codon_train_crops_labeled(C.byref(d), fake, 1 << 20, fake, fake, fake, None, None) == -1
    assert lib.codon_masked_l1_ssim_fwd(1, 8, 8, None, None, None, None, None, 1.0, 1.0, None, None, None, None, None) == -1
    assert b"masked_l1_ssim_fwd" in lib.codon_last_error_string()
    assert lib.codon_masked_l1_ssim_bwd(1, 6, 8, fake, fake, None, fake, fake, fake, fake, fake, None) == -2
