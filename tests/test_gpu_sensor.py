"""The sensor model of the training degradation on the MI355X.  The yardstick is the numpy restatement in
tests/sensor_ref.py (pinned on the CPU by tests/test_sensor_cpu.py and, through tools/host_check.py, equal byte for byte
to the kernel's own text compiled for the host); the bar is EQUAL BITS: codon_lr_sensor over every size, batch, level count,
mode, parameter set and hole pattern of sensor_ref.cases, its hole and snap properties, shards against one launch, the whole of
synthesize(sensor=...) against the composition of the existing restatements, and training that resumes bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from codon_amd import _lib as L
from codon_amd import infer, io, ops, train, upsample
from oracle import upsample_oracle as U
from tests import resample_masked_ref as M
from tests import sensor_ref as S
from tests import train_data_ref as R

pytestmark = pytest.mark.gpu

P_ = C.c_void_p
_tabs = {}


def _dev(key, make):
    if key not in _tabs:
        _tabs[key] = torch.from_numpy(np.ascontiguousarray(make())).cuda()
    return _tabs[key]


def _lut(levels):
    return M.tables(8 if levels == 255 else 16, levels)[1]


def _run(lr, masked, key, step, first, sigma, quad, edge_thr, p_drop, p_edge, levels):
    """codon_lr_sensor on the map lr (numpy, (B,1,p,p)); the output starts as -7 everywhere."""
    lib = L.load()
    src = torch.from_numpy(np.ascontiguousarray(lr)).cuda()
    B, _, p, _ = src.shape
    out = torch.full_like(src, -7.0)
    d = L.SensorDesc()
    d.batch, d.size, d.masked, d.seed_lo, d.seed_hi, d.step, d.first_sample = B, p, masked, key[0], key[1], step, first
    d.sigma, d.quad, d.edge_thr, d.p_drop, d.p_edge = sigma, quad, edge_thr, p_drop, p_edge
    gauss, lut = _dev("gauss", upsample.gauss_table), _dev(levels, lambda: _lut(levels))
    L.check(lib.codon_lr_sensor(C.byref(d), P_(src.data_ptr()), P_(gauss.data_ptr()), P_(lut.data_ptr()), levels,
                                P_(out.data_ptr()), ops._stream(src.device)), "lr_sensor")
    return out.cpu().numpy()


def _run_case(c, lr):
    return _run(lr, c["masked"], S.KEY, c["step"], c["first"], c["sigma"], c["quad"], c["edge_thr"], c["p_drop"], c["p_edge"], c["levels"])


def _bits_equal(got, ref, what):
    g = got.cpu().numpy() if torch.is_tensor(got) else got
    assert g.shape == ref.shape and g.dtype == ref.dtype == np.float32, (what, g.shape, ref.shape, g.dtype)
    bad = np.argwhere(g.view(np.uint32) != ref.view(np.uint32))
    assert bad.size == 0, f"{what}: {len(bad)} values differ, first at {bad[:3].tolist()}"


# ---- the kernel ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("p", S.SIZES)
@pytest.mark.parametrize("B", S.BATCHES)
def test_bit_identical_to_the_restatement(B, p):
    """Every case of sensor_ref.cases for this (B, p): levels 255 / 1000 / 65535, masked and unmasked, noise only, quad only,
    dropout only, edge dropout only and all together, no holes / scattered holes / a hole block on the border, steps 0, 1 and
    one above 2^31, first sample 0 and 37."""
    n = 0
    for c in S.cases(B, p):
        lr = S.input_map(B, p, c["kind"], c["levels"], c["masked"], c["seed"])
        got = _run_case(c, lr)
        _bits_equal(got, S.run_case(c, lr), c["name"])
        if c["masked"]:                                                   # a hole stays a hole: +0.0f on the bits
            assert not got.view(np.uint32)[lr == 0].any(), c["name"]
        n += 1
    assert n == 72
    assert {c["step"] for c in S.cases(B, p)} == set(S.STEPS) and {c["first"] for c in S.cases(B, p)} == set(S.FIRSTS)


def test_hole_and_snap_properties():
    B, p = 5, 33
    for levels in S.LEVELS:
        lut = _lut(levels)
        lr = S.input_map(B, p, "pattern", levels, 1, seed=levels)
        lr[:, :, :2, :17] = 0                                              # and a block on the border
        # noise far wider than the grid, with dropout: a pixel comes out 0 exactly where it was a hole or was dropped
        args = (1, S.KEY, 7, 3, np.float32(0.5), np.float32(0.25), np.float32(0.5), 0.2, 0.3)
        got = _run(lr, *args, levels)
        ref, hole, dropped, _, _ = S.sensor(lr, *args, levels, lut, with_parts=True)
        _bits_equal(got, ref, f"levels {levels}")
        assert hole.any() and dropped.any() and (~(hole | dropped)).any()
        assert not got.view(np.uint32)[hole | dropped].any()               # +0.0f, on the bits
        assert np.array_equal(got == 0, hole | dropped)                    # no other pixel is code 0 ...
        kept = got[~(hole | dropped)]
        assert kept.min() >= lut[1] and kept.max() <= lut[levels] and (kept == lut[1]).any() and (kept == lut[levels]).any()
        assert np.isin(kept.view(np.uint32), lut[:levels + 1].view(np.uint32)).all()      # ... and every one is on the grid
        # all parameters 0: the masked output is the input bit for bit, the unmasked one in value
        zero = (S.KEY, 7, 3, np.float32(0), np.float32(0), np.float32(0), 0.0, 0.0)
        _bits_equal(_run(lr, 1, *zero, levels), lr, f"levels {levels}: masked identity")
        free = S.input_map(B, p, "block", levels, 0, seed=1)
        assert np.array_equal(_run(free, 0, *zero, levels), free)


def test_shards_equal_one_launch():
    """The two halves of a batch of 8, first sample 0 and 4, concatenated, are the batch of 8 in one launch -- and the batch at
    first sample 4 is not the batch at 0."""
    lr = S.input_map(8, 7, "pattern", 255, 1, seed=4)
    args = (S.KEY, 11, np.float32(0.01), np.float32(0.02), np.float32(0.5), 0.1, 0.4, 255)
    one = _run(lr, 1, args[0], args[1], 0, *args[2:])
    halves = np.concatenate([_run(lr[:4], 1, args[0], args[1], 0, *args[2:]), _run(lr[4:], 1, args[0], args[1], 4, *args[2:])])
    _bits_equal(halves, one, "shards")
    assert not np.array_equal(_run(lr[4:], 1, args[0], args[1], 0, *args[2:]), one[4:])


# ---- synthesize --------------------------------------------------------------------------------------------------------------------

def _write_set(root, sizes, bits, depth_max, seed=0, smooth=False):
    """depth/ with scattered holes and one blob, color/: (dirs, [depth arrays])."""
    g = np.random.default_rng(seed)
    dd, cd = os.path.join(root, "depth"), os.path.join(root, "color")
    os.makedirs(dd)
    os.makedirs(cd)
    top = 255 if bits == 8 else depth_max
    wr = io.write_gray if bits == 8 else io.write_depth16
    deps = []
    for i, (h, w) in enumerate(sizes):
        yy, xx = np.mgrid[0:h, 0:w]
        v = 0.5 + 0.4 * np.sin(0.11 * yy + 0.3 * i) * np.cos(0.07 * xx) * (1.0 if smooth else np.sign(np.sin(0.23 * xx + 0.19 * yy)))
        dep = np.clip(np.rint(v * top), 1, top).astype(np.uint8 if bits == 8 else np.uint16)
        dep[M.holes(h, w, "pattern", seed=seed + i)] = 0
        if not smooth:
            dep[2 * h // 7:5 * h // 7, 2 * w // 7:5 * w // 7] = 0          # a blob wide enough to survive the reduction
        wr(os.path.join(dd, f"{i:02d}.png"), dep)
        io.write_gray(os.path.join(cd, f"{i:02d}.png"), np.clip(v * 255 + g.integers(-20, 21, size=(h, w)), 0, 255).astype(np.uint8))
        deps.append(dep)
    return (dd, cd), deps


@pytest.mark.parametrize("s, P", [(4, 16), (8, 64)])
@pytest.mark.parametrize("masked", [True, False])
@pytest.mark.parametrize("bits, depth_max", [(8, 255), (16, 10000)])
def test_synthesize_with_a_sensor_model(tmp_path, bits, depth_max, masked, s, P):
    """crop -> down -> sensor -> up -> quantise from the existing restatements; five launches in that order and no host
    synchronisation; y and t untouched; on the masked path x is what infer.codes_to_input builds from the noisy map's codes."""
    from tests.abi_log_8bit import _acl
    lv, lut = M.tables(bits, depth_max)
    (dd, cd), deps = _write_set(str(tmp_path), [(70, 81), (64, 90)], bits, depth_max, seed=bits + s)
    ts = train.TrainSet(dd, cd, "cuda:0", depth_bits=bits, depth_max=depth_max if bits == 16 else 65535)
    rows = []
    for b in range(5):
        h, w = ts.sizes[b % 2].tolist()
        y0, x0 = [(0, 0), (h - P, w - P), (0, w - P), (h - P, 0), ((h - P) // 2, (w - P) // 2)][b]
        rows.append([int(ts.offsets[b % 2]), h, w, y0, x0, (3 * b + 1) % 8])
    descs = np.asarray(rows, dtype=np.int64)
    model = train.SensorModel(noise=1.5, noise_quad=2.0, dropout=0.05 if masked else 0.0, edge_dropout=0.4 if masked else 0.0,
                              edge_threshold=20.0 * lv / 255, seed=(0xABCDEF << 32) | 99)
    kw = dict(degrade_holes=masked, sensor=model, step=(1 << 31) + 6, first_sample=11)
    train.synthesize(ts, descs, s, P, **kw)                               # the tables go up on first use
    torch.cuda.synchronize()
    real = L.load()
    log = _acl().install()
    torch.cuda.set_sync_debug_mode("error")
    try:
        x, y, t, lr = train.synthesize(ts, descs, s, P, return_lr=True, **kw)
    finally:
        torch.cuda.set_sync_debug_mode("default")
        L._lib = real
    names = [n for n, _, _ in log]
    crops, quant = ("codon_train_crops_u16", "codon_quantize_levels") if bits == 16 else ("codon_train_crops", "codon_quantize_u8")
    tail = "_masked" if masked else ""
    assert names == [crops, "codon_bicubic_downsample" + tail, "codon_lr_sensor", "codon_bicubic_upsample" + tail, quant], names
    assert log[2][1][0] == {"batch": 5, "size": P // s, "masked": int(masked), "seed_lo": 99, "seed_hi": 0xABCDEF,
                            "step": (1 << 31) + 6, "first_sample": 11, "sigma": float(S.units(1.5, lv)),
                            "quad": float(S.units(2.0, lv)), "edge_thr": float(S.units(20.0 * lv / 255, lv)), "reserved_f": 0.0,
                            "p_drop": model.dropout, "p_edge": model.edge_dropout} and log[2][1][4] == lv
    px, py, pt = train.synthesize(ts, descs, s, P, degrade_holes=masked)
    assert torch.equal(y, py) and torch.equal(t, pt) and not torch.equal(x, px)
    by_off = {int(o): d for o, d in zip(ts.offsets, deps)}
    src = np.stack([lut[R.d4(by_off[off][y0:y0 + P, x0:x0 + P], op).astype(np.int64)] for off, _, _, y0, x0, op in descs.tolist()])[:, None]
    _bits_equal(t, src, "source")
    clean = M.downsample_masked(src, s, lv, lut) if masked else R.downsample(src, s)
    rlr = S.sensor(clean, int(masked), (99, 0xABCDEF), (1 << 31) + 6, 11, S.units(1.5, lv), S.units(2.0, lv),
                   S.units(20.0 * lv / 255, lv), model.dropout, model.edge_dropout, lv, lut)
    rup = M.upsample_masked(rlr, s)[0] if masked else U.bicubic_upsample(rlr, s)
    _bits_equal(lr, rlr, "the noisy low-resolution map")
    _bits_equal(x, M.quantize(rup, lv, lut), "x")
    assert not np.array_equal(rlr, clean)
    if masked:
        assert ((rlr == 0) & (clean != 0)).any() and ((rlr != 0) & (rlr != clean)).any()        # dropout and noise both bite
        codes = np.rint(rlr[:, 0].astype(np.float64) * lv).astype(np.int64)
        assert np.array_equal(np.asarray(lut)[codes].view(np.uint32), rlr[:, 0].view(np.uint32))      # the map IS on the code grid
        host = codes.astype(np.uint8) if bits == 8 else codes.astype(np.uint16).view(np.int16)
        assert torch.equal(x, infer.codes_to_input(torch.from_numpy(host).cuda(), s, torch.float32, depth_max if bits == 16 else None))


# ---- training ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_fit_with_a_model_resumes_bit_identically(tmp_path, dtype):
    (dd, cd), _ = _write_set(str(tmp_path), [(48, 40), (40, 52), (44, 44)], 8, 255, seed=2, smooth=True)
    base = ["--scale", "4", "--train-depth", dd, "--train-color", cd, "--mask-holes", "--degrade-holes", "--crop", "32", "--batch", "2",
            "--log-every", "1", "--seed", "5", "--dtype", dtype]
    cli = lambda *extra: base + ["--sensor-noise", "2", "--sensor-noise-quad", "1", "--sensor-dropout", "0.05",                # noqa: E731
                                 "--sensor-edge-dropout", "0.3", "--sensor-edge-threshold", "6", *extra]
    a, b, c = (str(tmp_path / n) for n in ("a.pth", "b.pth", "c.pth"))
    quiet = lambda s: None                                               # noqa: E731
    straight = train.main(cli("--steps", "4", "--save", a), emit=quiet)
    train.main(cli("--steps", "2", "--save", b), emit=quiet)
    resumed = train.main(cli("--steps", "4", "--resume", b, "--save", c), emit=quiet)
    assert [s for s, _ in resumed["losses"]] == [3, 4] and resumed["losses"] == straight["losses"][2:]
    assert all(np.isfinite(v) for _, v in straight["losses"]) and straight["losses"][0][0] == 1
    ca, cc = torch.load(a, weights_only=False), torch.load(c, weights_only=False)
    assert ca["epoch"] == cc["epoch"] == 4 and ca["rng"] == cc["rng"]
    assert {k: ca["args"][k] for k in train.SENSOR_DEFAULTS} == {k: cc["args"][k] for k in train.SENSOR_DEFAULTS} == \
        train.SensorModel(2.0, 1.0, 0.05, 0.3, 6.0, 5).args()
    for k, v in ca["model"].items():
        assert torch.equal(v, cc["model"][k]), k
    for k in ("exp_avg", "exp_avg_sq"):
        assert torch.equal(ca["optimizer"][k], cc["optimizer"][k]), k
    for p, q in zip(straight["gs"].params, resumed["gs"].params):
        assert torch.equal(p, q)
    with pytest.raises(ValueError, match="sensor_dropout 0.05 != None"):
        train.main(base + ["--steps", "4", "--resume", b], emit=quiet)     # refused before any GPU work


def test_the_seed_decides_the_maps(tmp_path):
    """Same descriptors, same weights: two runs whose models differ in the seed only feed the network another x at step 1 (and
    at step 2 another one than at step 1); the same seed feeds it the same x."""
    from codon_amd import CODONNet
    (dd, cd), _ = _write_set(str(tmp_path), [(48, 40), (40, 52)], 8, 255, seed=3, smooth=True)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32)
    fixed = train.draw(np.random.default_rng(1), ts, 2, 32)

    def xs(seed):
        torch.manual_seed(0)
        m = CODONNet().cuda()
        seen = []
        h = m.register_forward_pre_hook(lambda mod, inp: seen.append(inp[0].detach().clone()))
        train.fit(m, ts, 2, scale=4, crop=32, batch=2, dtype="bf16", fixed=fixed, emit=lambda s: None, degrade_holes=True,
                  sensor=train.SensorModel(noise=2.0, dropout=0.05, seed=seed))
        h.remove()
        assert len(seen) == 2
        return seen

    a, b, c = xs(5), xs(5), xs(6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert not torch.equal(a[0], c[0]) and not torch.equal(a[0], a[1])
    want = train.synthesize(ts, fixed, 4, 32, degrade_holes=True, sensor=train.SensorModel(noise=2.0, dropout=0.05, seed=5), step=1)[0]
    assert torch.equal(a[0].float(), want)


def test_a_rank_builds_its_shard_of_the_global_batch(tmp_path, monkeypatch):
    """What fit hands the network on rank r of 2 -- the rank and world size it is told, no second process: the step is cut short
    at the forward -- is samples 2r and 2r + 1 of the batch of 4 that one process builds; with the shard start left at 0, rank 1
    would have drawn rank 0's noise."""
    from codon_amd import CODONNet
    (dd, cd), _ = _write_set(str(tmp_path), [(48, 40), (40, 52)], 8, 255, seed=3, smooth=True)
    ts = train.TrainSet(dd, cd, "cuda:0", crop=32)
    model = train.SensorModel(noise=2.0, dropout=0.05, seed=8)

    class Stop(Exception):
        pass

    def first_x(rank, world):
        monkeypatch.setattr(train, "_world", lambda group: (rank, world))
        m = CODONNet().cuda()
        seen = []

        def hook(mod, inp):
            seen.append(inp[0].detach().clone())
            raise Stop

        m.register_forward_pre_hook(hook)
        with pytest.raises(Stop):
            train.fit(m, ts, 1, scale=4, crop=32, batch=4, seed=9, emit=lambda s: None, degrade_holes=True, sensor=model)
        return seen[0]

    whole = first_x(0, 1)
    assert whole.shape == (4, 1, 32, 32)
    for rank in (0, 1):
        assert torch.equal(first_x(rank, 2), whole[2 * rank:2 * rank + 2]), rank
    descs = train.draw(np.random.default_rng(9), ts, 4, 32, 1, 2)
    unsharded = train.synthesize(ts, descs, 4, 32, degrade_holes=True, sensor=model, step=1, first_sample=0)[0]
    assert not torch.equal(unsharded, whole[2:4])
    assert torch.equal(train.synthesize(ts, descs, 4, 32, degrade_holes=True, sensor=model, step=1, first_sample=2)[0], whole[2:4])
