"""The sensor model of the training degradation, what needs no GPU: Philox4x32-10 in the library and in the numpy
restatement against the published known-answer vectors, the Gaussian table, the statistics of the definition (on the
restatement alone), every host-side refusal of codon_lr_sensor, of synthesize, of fit and of the command line, the
checkpoint keys.  (The host-side sanitizer check of the kernel's own text: tests/test_tools_host_checks.py.)"""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import io, train, upsample
from tests import sensor_ref as S


# ---- the generator ---------------------------------------------------------------------------------------------------------------

def test_philox_known_answers():
    lib = L.load()
    for ctr, key, want in S.KAT:
        c, k, o = (C.c_uint32 * 4)(*ctr), (C.c_uint32 * 2)(*key), (C.c_uint32 * 4)()
        assert lib.codon_philox4x32_10(c, k, o) == 0
        assert tuple(o) == want, [hex(v) for v in o]
        assert tuple(int(w) for w in S.philox(*ctr, *key)) == want
    # arrays: the restatement word by word against the library on counters of the kernel's layout
    w = S.words(2, 4, (12345, 7), (1 << 31) + 3, first=5)
    for b, y, x in ((0, 0, 0), (1, 3, 2), (0, 2, 3)):
        c, k, o = (C.c_uint32 * 4)(y * 4 + x, 5 + b, (1 << 31) + 3, 0), (C.c_uint32 * 2)(12345, 7), (C.c_uint32 * 4)()
        assert lib.codon_philox4x32_10(c, k, o) == 0
        assert tuple(o) == tuple(int(v[b, 0, y, x]) for v in w)
    p = (C.c_uint32 * 4)()
    assert lib.codon_philox4x32_10(None, (C.c_uint32 * 2)(), p) == -1 and b"philox4x32_10: null pointer" in lib.codon_last_error_string()
    assert lib.codon_philox4x32_10(p, None, p) == -1 and lib.codon_philox4x32_10(p, (C.c_uint32 * 2)(), None) == -1


# ---- the table -------------------------------------------------------------------------------------------------------------------

def test_gauss_table():
    g = upsample.gauss_table()
    assert g.dtype == np.float32 and g.shape == (65536,)
    assert np.array_equal(g, -g[::-1])                                    # exactly antisymmetric
    assert (np.diff(g) > 0).all()                                         # strictly increasing
    again = upsample.gauss_table.__wrapped__()                            # a second build, past the cache
    assert again is not g and np.array_equal(again.view(np.uint32), g.view(np.uint32))
    assert np.array_equal(S.gauss_table().view(np.uint32), g.view(np.uint32))
    assert abs(float(g[-1]) - 4.3249) < 1e-4 and float(g.astype(np.float64).mean()) == 0.0
    std = float(g.astype(np.float64).std())
    print(f"float64 std of the table {std:.8f} (bar: within 2e-5 of 1)")
    assert abs(std - 1.0) < 2e-5


# ---- the definition's statistics, on the restatement alone -----------------------------------------------------------------------

def test_reference_statistics():
    B, p, key, step = 8, 64, (12345, 0), 3
    n = B * p * p
    w0, w1, _, _ = S.words(B, p, key, step)
    g = S.gauss_table()[(w0 >> np.uint64(16)).astype(np.int64)].astype(np.float64)
    mean, std = float(g.mean()), float(g.std())
    print(f"n {n}: mean {mean:.4f} (bar {5 / math.sqrt(n):.4f}), std {std:.4f} (bar +-{5 / math.sqrt(2 * n) + 2e-5:.4f})")
    assert abs(mean) < 5 / math.sqrt(n)
    assert abs(std - 1.0) < 5 / math.sqrt(2 * n) + 2e-5
    lut = S.M.tables(8)[1]
    flat = np.full((B, 1, p, p), lut[128], dtype=np.float32)              # no hole, no edge: plain dropout
    for P in (0.05, 0.25):
        _, hole, dropped, e, _ = S.sensor(flat, 1, key, step, 0, 0.0, 0.0, 0.0, P, 0.0, 255, lut, with_parts=True)
        assert not hole.any() and not e.any()
        z = (dropped.mean() - P) / math.sqrt(P * (1 - P) / n)
        print(f"P {P}: dropped {dropped.mean():.5f}, z {z:.2f} (bar 5)")
        assert abs(z) < 5
        assert np.array_equal(dropped, w1 < np.uint64(S.threshold(P)))
    rh = float(np.corrcoef(g[..., :-1].reshape(-1), g[..., 1:].reshape(-1))[0, 1])
    rs = float(np.corrcoef(g[0].reshape(-1), g[1].reshape(-1))[0, 1])
    print(f"correlation: horizontal neighbours {rh:.3f}, samples 0 and 1 {rs:.3f} (bar 0.05)")
    assert abs(rh) < 0.05 and abs(rs) < 0.05
    # P = 0 never drops, P = 1 always does; the edge term adds its threshold where there is an edge only
    assert S.threshold(0.0) == 0 and S.threshold(1.0) == 1 << 32 and S.threshold(0.5) == 1 << 31
    for P, want in ((0.0, False), (1.0, True)):
        d = S.sensor(flat, 1, key, step, 0, 0.0, 0.0, 0.0, P, 0.0, 255, lut, with_parts=True)[2]
        assert bool(d.all()) is want and bool(d.any()) is want
    step_map = flat.copy()
    step_map[..., p // 2:] = lut[200]                                     # one vertical edge of 72 codes
    _, _, d, e, _ = S.sensor(step_map, 1, key, step, 0, 0.0, 0.0, S.units(50, 255), 0.0, 1.0, 255, lut, with_parts=True)
    assert np.array_equal(e[0, 0].any(0), np.isin(np.arange(p), (p // 2 - 1, p // 2))) and np.array_equal(d, e)


# ---- codon_lr_sensor's refusals, on the host -------------------------------------------------------------------------------------

def test_lr_sensor_refusals_without_gpu():
    lib = L.load()
    fake, other = C.c_void_p(4096), C.c_void_p(1 << 20)                   # never dereferenced: every call is refused on the host

    def call(lr=fake, gauss=fake, lut=fake, levels=255, out=other, desc=True, **f):
        d = L.SensorDesc()
        d.batch, d.size, d.masked = 4, 8, 1
        for k, v in f.items():
            setattr(d, k, v)
        st = lib.codon_lr_sensor(C.byref(d) if desc else None, lr, gauss, lut, levels, out, None)
        return st, lib.codon_last_error_string().decode()

    for kw in ({"lr": None}, {"gauss": None}, {"lut": None}, {"out": None}, {"desc": False}):
        assert call(**kw) == (-1, "lr_sensor: null pointer"), kw
    assert call(out=fake)[0] == -1 and "same buffer" in call(out=fake)[1]
    for bad, word in ((dict(batch=0), "batch 0 "), (dict(batch=L.TRAIN_MAX_BATCH + 1), "batch 65 "), (dict(size=3), "size 3 "),
                      (dict(size=513), "size 513 "), (dict(levels=0), "levels 0 "), (dict(levels=65536), "levels 65536 "),
                      (dict(step=-1), "step -1 "), (dict(step=1 << 32), "step 4294967296 "), (dict(first_sample=-1), "first_sample -1 "),
                      (dict(first_sample=(1 << 32) - 3), "first_sample 4294967293 "),
                      (dict(sigma=-1.0), "sigma -1 "), (dict(sigma=math.inf), "sigma inf "), (dict(sigma=math.nan), "sigma nan "),
                      (dict(quad=-0.5), "quad -0.5 "), (dict(quad=math.inf), "quad inf "), (dict(quad=math.nan), "quad nan "),
                      (dict(edge_thr=-2.0), "edge_thr -2 "), (dict(edge_thr=math.inf), "edge_thr inf "),
                      (dict(edge_thr=math.nan), "edge_thr nan "),
                      (dict(p_drop=-0.1), "p_drop -0.1 "), (dict(p_drop=1.5), "p_drop 1.5 "), (dict(p_drop=math.nan), "p_drop nan "),
                      (dict(p_edge=-0.1), "p_edge -0.1 "), (dict(p_edge=1.5), "p_edge 1.5 "), (dict(p_edge=math.nan), "p_edge nan "),
                      (dict(p_drop=0.6, p_edge=0.5), "p_drop + p_edge = 1.1 "),
                      (dict(masked=0, p_drop=0.1), "masked 0 with p_drop 0.1"), (dict(masked=0, p_edge=0.2), "p_edge 0.2 ")):
        st, msg = call(**bad)
        assert st == -1 and msg.startswith("lr_sensor: ") and word in msg, (bad, msg)


# ---- SensorModel, synthesize, fit ------------------------------------------------------------------------------------------------

def _write_set(root, lr=False):
    g = np.random.default_rng(1)
    dirs = [os.path.join(root, n) for n in ("depth", "color", "lr")]
    for d in dirs:
        os.makedirs(d)
    io.write_gray(os.path.join(dirs[0], "00.png"), g.integers(1, 256, size=(40, 48)).astype(np.uint8))
    io.write_gray(os.path.join(dirs[1], "00.png"), g.integers(0, 256, size=(40, 48)).astype(np.uint8))
    if lr:
        io.write_gray(os.path.join(dirs[2], "00.png"), g.integers(0, 256, size=(10, 12)).astype(np.uint8))
    return dirs


def test_sensor_model_and_synthesize_refusals(tmp_path):
    m = train.SensorModel(noise=2.0, dropout=0.1, seed=7)
    assert (m.noise, m.noise_quad, m.dropout, m.edge_dropout, m.edge_threshold, m.seed) == (2.0, 0.0, 0.1, 0.0, 0.0, 7)
    with pytest.raises(Exception):                                        # frozen
        m.noise = 3.0
    assert set(m.args()) == set(train.SENSOR_DEFAULTS) and all(v is None for v in train.SENSOR_DEFAULTS.values())
    for bad in (dict(noise=-1.0), dict(noise=math.inf), dict(noise=math.nan), dict(noise_quad=-0.1), dict(noise_quad=math.nan),
                dict(edge_threshold=-1.0), dict(edge_threshold=math.inf), dict(dropout=-0.1), dict(dropout=1.1),
                dict(dropout=math.nan), dict(edge_dropout=2.0), dict(edge_dropout=math.nan), dict(dropout=0.6, edge_dropout=0.6),
                dict(seed=-1), dict(seed=1 << 64), dict(seed=1.5)):
        with pytest.raises(ValueError, match="SensorModel: "):
            train.SensorModel(**bad)
    dd, cd, ld = _write_set(str(tmp_path / "a"))
    ts = train.TrainSet(dd, cd, "cpu")
    descs = np.asarray([[0, 40, 48, 0, 0, 0]], dtype=np.int64)
    for model in (train.SensorModel(dropout=0.1), train.SensorModel(edge_dropout=0.1, edge_threshold=5.0)):
        with pytest.raises(ValueError, match="synthesize: sensor dropout needs degrade_holes"):
            train.synthesize(ts, descs, 4, 32, sensor=model)
        with pytest.raises(ValueError, match="fit: sensor dropout needs degrade_holes"):
            train.fit(None, ts, 1, scale=4, crop=32, batch=1, sensor=model)
    for kw in (dict(step=-1), dict(step=1 << 32), dict(first_sample=-1), dict(first_sample=1 << 32)):
        with pytest.raises(ValueError, match="must fit 32 bits"):
            train.synthesize(ts, descs, 4, 32, sensor=train.SensorModel(noise=1.0), **kw)
    dd, cd, ld = _write_set(str(tmp_path / "b"), lr=True)
    tl = train.TrainSet(dd, cd, "cpu", lr_dir=ld, scale=4)
    with pytest.raises(ValueError, match="synthesize: a sensor model does not go with a TrainSet of low-resolution maps"):
        train.synthesize(tl, descs, 4, 32, sensor=train.SensorModel(noise=1.0))
    with pytest.raises(ValueError, match="fit: a sensor model does not go with a TrainSet of low-resolution maps"):
        train.fit(None, tl, 1, scale=4, crop=32, batch=1, sensor=train.SensorModel(noise=1.0))


# ---- the command line and the checkpoint keys ------------------------------------------------------------------------------------

PARENT_ARG_KEYS = {"scale", "crop", "batch", "dtype", "lr", "seed", "clip_norm", "skip_nonfinite", "ema", "lr_schedule",
                   "warmup_steps", "lr_min", "lr_steps", "mask_holes", "min_valid", "train_label"}


def _argv(*extra):
    return ["--scale", "4", "--train-depth", "d", "--train-color", "c", *extra]


def test_cli_refusals(capsys):
    def refused(*extra):
        with pytest.raises(SystemExit):
            train.parse_args(_argv(*extra))
        return capsys.readouterr().err

    assert "--sensor-dropout needs --degrade-holes" in refused("--sensor-dropout", "0.1")
    assert "--sensor-edge-dropout needs --degrade-holes" in refused("--sensor-edge-dropout", "0.1", "--sensor-edge-threshold", "4")
    for opt in ("--sensor-noise", "--sensor-noise-quad"):
        assert f"{opt} and --train-lr-depth exclude each other" in refused(opt, "1", "--train-lr-depth", "l")
    assert "--train-lr-depth exclude each other" in refused("--sensor-dropout", "0.1", "--train-lr-depth", "l")
    assert "--sensor-edge-threshold go together" in refused("--degrade-holes", "--sensor-edge-dropout", "0.1")
    assert "--sensor-edge-threshold go together" in refused("--degrade-holes", "--sensor-edge-threshold", "4")
    for opt in ("--sensor-noise", "--sensor-noise-quad", "--sensor-dropout"):
        for v in ("-1", "nan", "inf", "-inf"):
            assert f"{opt} {float(v)} must be finite and not negative" in refused("--degrade-holes", f"{opt}={v}"), (opt, v)
    for v in ("-1", "nan", "inf"):
        for pair in ((f"--sensor-edge-dropout={v}", "--sensor-edge-threshold=4"), ("--sensor-edge-dropout=0.1", f"--sensor-edge-threshold={v}")):
            assert "must be finite and not negative" in refused("--degrade-holes", *pair), pair
    assert "together at most 1" in refused("--degrade-holes", "--sensor-dropout", "1.5")
    assert "together at most 1" in refused("--degrade-holes", "--sensor-dropout", "0.6", "--sensor-edge-dropout", "0.5",
                                           "--sensor-edge-threshold", "4")
    assert "--seed -1" in refused("--sensor-noise", "1", "--seed", "-1")
    a = train.parse_args(_argv("--degrade-holes", "--sensor-noise", "1.5", "--sensor-noise-quad", "3", "--sensor-dropout", "0.05",
                               "--sensor-edge-dropout", "0.3", "--sensor-edge-threshold", "12", "--seed", "9"))
    assert train.sensor_of(a) == train.SensorModel(1.5, 3.0, 0.05, 0.3, 12.0, 9)
    assert train.sensor_of(train.parse_args(_argv("--sensor-noise", "2"))) == train.SensorModel(noise=2.0)     # noise alone: either path
    assert train.sensor_of(train.parse_args(_argv())) is None


def test_resume_keys(tmp_path):
    plain = train.run_args(train.parse_args(_argv()))
    assert set(plain) == PARENT_ARG_KEYS                                   # no model: exactly the keys checkpoints always had
    on = train.run_args(train.parse_args(_argv("--sensor-noise", "2", "--seed", "3")))
    assert set(on) == PARENT_ARG_KEYS | set(train.SENSOR_DEFAULTS)
    assert {k: on[k] for k in train.SENSOR_DEFAULTS} == {"sensor_noise": 2.0, "sensor_noise_quad": 0.0, "sensor_dropout": 0.0,
                                                          "sensor_edge_dropout": 0.0, "sensor_edge_threshold": 0.0, "sensor_seed": 3}
    ck = {"epoch": 2, "model": {}, "optimizer": {}, "rng": np.random.default_rng(0).bit_generator.state}
    p = str(tmp_path / "ck.pth")
    torch.save(dict(ck, args=plain), p)                                    # a checkpoint without the keys: "no model"
    assert train.load_resume(p, plain)["epoch"] == 2
    with pytest.raises(ValueError, match="other arguments: sensor_noise None != 2.0"):
        train.load_resume(p, on)
    torch.save(dict(ck, args=on), p)
    assert train.load_resume(p, on)["epoch"] == 2
    with pytest.raises(ValueError, match="sensor_noise 2.0 != 2.5"):
        train.load_resume(p, dict(on, sensor_noise=2.5))
    with pytest.raises(ValueError, match="sensor_seed 3 != 4"):
        train.load_resume(p, train.run_args(train.parse_args(_argv("--sensor-noise", "2", "--seed", "4"))))
    with pytest.raises(ValueError, match="sensor_noise 2.0 != None"):
        train.load_resume(p, plain)
    with pytest.raises(ValueError, match="sensor_noise 2.0 != None"):
        train.main(_argv("--resume", p))                                   # refused before any device or file work
