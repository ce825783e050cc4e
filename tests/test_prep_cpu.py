"""The record of the low-resolution depth preparation (codon_amd/prep.py) without a GPU: which combinations of its
four options it accepts and in which words it refuses the others, that set_options() holds exactly the options that are set and
from_mapping() inverts it, that the training command line still writes the checkpoint keys it always wrote, and the one table of
resume keys.  What is expected is spelled out here, not worked out from the code under test."""
import pytest

from codon_amd import train
from codon_amd.prep import LrPrep

S = 3.0                     # the sigma of a row that gives one
# (low-resolution codes given, fill_holes, fill_guided, fill_sigma given, normalize) -> set_options() of the record, or the refusal
# of a caller "who" whose low-resolution argument is called "lr_depth"
NEEDS_LR = "who: fill_holes needs lr_depth (only low-resolution code planes are filled)"
NEEDS_FILL = "who: fill_guided needs fill_holes (it chooses how the holes are filled)"
NORM_NEEDS_LR = "who: normalize needs lr_depth (input_depth maps are not code planes: only low-resolution codes are normalised)"
TABLE = [
    (1, 0, 0, 0, 0, {}),
    (1, 0, 0, 0, 1, {"normalize": True}),
    (1, 0, 0, 1, 0, {}),                                                            # a sigma without fill_guided is not an option
    (1, 0, 0, 1, 1, {"normalize": True}),
    (1, 0, 1, 0, 0, NEEDS_FILL),
    (1, 0, 1, 0, 1, NEEDS_FILL),
    (1, 0, 1, 1, 0, NEEDS_FILL),
    (1, 0, 1, 1, 1, NEEDS_FILL),
    (1, 1, 0, 0, 0, {"fill_holes": True}),
    (1, 1, 0, 0, 1, {"fill_holes": True, "normalize": True}),
    (1, 1, 0, 1, 0, {"fill_holes": True}),
    (1, 1, 0, 1, 1, {"fill_holes": True, "normalize": True}),
    (1, 1, 1, 0, 0, {"fill_holes": True, "fill_guided": True, "fill_sigma": 10.0}),
    (1, 1, 1, 0, 1, {"fill_holes": True, "fill_guided": True, "fill_sigma": 10.0, "normalize": True}),
    (1, 1, 1, 1, 0, {"fill_holes": True, "fill_guided": True, "fill_sigma": 3.0}),
    (1, 1, 1, 1, 1, {"fill_holes": True, "fill_guided": True, "fill_sigma": 3.0, "normalize": True}),
    (0, 0, 0, 0, 0, {}),
    (0, 0, 0, 0, 1, NORM_NEEDS_LR),
    (0, 0, 0, 1, 0, {}),
    (0, 0, 0, 1, 1, NORM_NEEDS_LR),
    (0, 0, 1, 0, 0, NEEDS_FILL),
    (0, 0, 1, 0, 1, NEEDS_FILL),
    (0, 0, 1, 1, 0, NEEDS_FILL),
    (0, 0, 1, 1, 1, NEEDS_FILL),
    (0, 1, 0, 0, 0, NEEDS_LR),
    (0, 1, 0, 0, 1, NEEDS_LR),
    (0, 1, 0, 1, 0, NEEDS_LR),
    (0, 1, 0, 1, 1, NEEDS_LR),
    (0, 1, 1, 0, 0, NEEDS_LR),
    (0, 1, 1, 0, 1, NEEDS_LR),
    (0, 1, 1, 1, 0, NEEDS_LR),
    (0, 1, 1, 1, 1, NEEDS_LR),
]


def _kw(fill, guided, sigma, norm):
    return dict(fill_holes=bool(fill), fill_guided=bool(guided), normalize=bool(norm), **({"fill_sigma": S} if sigma else {}))


def test_every_combination_is_built_or_refused_by_name():
    assert len({row[:5] for row in TABLE}) == 32
    for has_lr, fill, guided, sigma, norm, want in TABLE:
        kw = _kw(fill, guided, sigma, norm)
        if isinstance(want, str):
            with pytest.raises(ValueError) as e:
                LrPrep.checked("who", lr=("lr_depth", bool(has_lr)), **kw)
            assert str(e.value) == want, (has_lr, kw)
            continue
        p = LrPrep.checked("who", lr=("lr_depth", bool(has_lr)), **kw)
        assert p.set_options() == want, (has_lr, kw)
        assert (p.fill_holes, p.fill_guided, p.normalize) == (bool(fill), bool(guided), bool(norm))
        assert p.fill_sigma == (S if guided and sigma else 10.0) and isinstance(p.fill_sigma, float)
        assert LrPrep.from_mapping(want) == p == LrPrep(**want)                     # the inverse of set_options()
        assert LrPrep.from_mapping(dict(want, scale=4, color="c", every=1)) == p    # a `val` dict: other keys are not looked at
    assert LrPrep() == LrPrep.from_mapping({}) == LrPrep.from_mapping({"fill_holes": None, "fill_sigma": None})
    assert LrPrep().set_options() == {}
    with pytest.raises(Exception):
        LrPrep().fill_holes = True                                                  # frozen


def test_the_callers_own_rules():
    # a caller that stretches other planes too (TrainSet: the depth plane of a set without low-resolution maps)
    assert LrPrep.checked("TrainSet", normalize=True, lr=("lr_dir", False), normalize_needs_lr=False).set_options() == {"normalize": True}
    with pytest.raises(ValueError, match="TrainSet: fill_holes needs lr_dir"):
        LrPrep.checked("TrainSet", fill_holes=True, normalize=True, lr=("lr_dir", False), normalize_needs_lr=False)
    # a caller with rules of its own about where the options apply (fit): the values are checked, the combinations are not
    assert LrPrep.checked("fit", fill_guided=True, fill_sigma=4).set_options() == {"fill_guided": True, "fill_sigma": 4.0}
    for bad in (0, -1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError, match=r"fit: fill_sigma .* \(a positive number of guidance codes\)"):
            LrPrep.checked("fit", fill_holes=True, fill_guided=True, fill_sigma=bad)
        assert LrPrep.checked("fit", fill_holes=True, fill_sigma=bad).fill_sigma == 10.0          # not looked at without fill_guided
    # the grid the stretch needs
    with pytest.raises(ValueError, match="who: normalize: depth_max 1 leaves per-image normalisation no grid"):
        LrPrep.checked("who", normalize=True, lr=("lr_depth", True), top=1)
    assert LrPrep.checked("who", normalize=True, lr=("lr_depth", True), top=2).normalize
    assert LrPrep.checked("who", fill_holes=True, lr=("lr_depth", True), top=1).fill_holes       # nothing is stretched


# ---- the training command line writes the keys it always wrote -------------------------------------------------------------------

BASE = {"scale": 4, "crop": 128, "batch": 16, "dtype": "bf16", "lr": 1e-4, "seed": 0, "clip_norm": None, "skip_nonfinite": False,
        "ema": None, "lr_schedule": "constant", "warmup_steps": 0, "lr_min": 0.0, "lr_steps": None, "mask_holes": False,
        "min_valid": 0.0, "train_label": False, "train_lr_depth": True}
FLAGS = ("--fill-holes", "--fill-guided", ("--fill-sigma", "3"), "--normalize")
REFUSED = {(0, 0, 1): "--fill-sigma needs --fill-guided", (1, 0, 1): "--fill-sigma needs --fill-guided",
           (0, 1, 0): "--fill-guided needs --train-lr-depth --fill-holes", (0, 1, 1): "--fill-guided needs --train-lr-depth --fill-holes"}


def test_run_args_of_every_combination(capsys):
    for has_lr, fill, guided, sigma, norm, want in TABLE[:16]:
        argv = ["--scale", "4", "--train-depth", "d", "--train-color", "c", "--train-lr-depth", "l"]
        for on, flag in zip((fill, guided, sigma, norm), FLAGS):
            argv += ([flag] if isinstance(flag, str) else list(flag)) if on else []
        word = REFUSED.get((fill, guided, sigma))
        if word is not None:
            with pytest.raises(SystemExit):
                train.parse_args(argv)
            assert word in capsys.readouterr().err, argv
            continue
        a = train.parse_args(argv)
        assert (a.fill_holes, a.fill_guided, a.normalize) == (bool(fill), bool(guided), bool(norm))
        assert a.fill_sigma == (3.0 if sigma else 10.0)
        assert train.run_args(a) == {**BASE, **want}, argv
    # the synthetic path: filled every step by synthesize, and the key is the same
    a = train.parse_args(["--scale", "4", "--train-depth", "d", "--train-color", "c", "--degrade-holes", "--fill-holes", "--normalize"])
    assert train.run_args(a) == {**{k: v for k, v in BASE.items() if k != "train_lr_depth"}, "degrade_holes": True,
                                 "fill_holes": True, "normalize": True}


def test_one_resume_table():
    later = ("depth_bits", "depth_max", "degrade_holes", "train_lr_depth", "sensor_noise", "sensor_noise_quad", "sensor_dropout",
             "sensor_edge_dropout", "sensor_edge_threshold", "sensor_seed", "fill_holes", "fill_guided", "fill_sigma", "normalize")
    assert train.RESUME_ALL_KEYS == train.RESUME_KEYS + later
    assert later == sum((tuple(d) for d in (train.DEPTH_DEFAULTS, train.DEGRADE_DEFAULTS, train.LR_DEFAULTS, train.SENSOR_DEFAULTS,
                                            train.FILL_DEFAULTS, train.GUIDED_DEFAULTS, train.NORM_DEFAULTS)), ())
    assert train.RESUME_ALL_DEFAULTS == {
        "clip_norm": None, "skip_nonfinite": False, "ema": None, "lr_schedule": "constant", "warmup_steps": 0, "lr_min": 0.0,
        "lr_steps": None, "mask_holes": False, "min_valid": 0.0, "train_label": False, "depth_bits": 8, "depth_max": 65535,
        "degrade_holes": False, "train_lr_depth": False, "sensor_noise": None, "sensor_noise_quad": None, "sensor_dropout": None,
        "sensor_edge_dropout": None, "sensor_edge_threshold": None, "sensor_seed": None, "fill_holes": False, "fill_guided": False,
        "fill_sigma": 10.0, "normalize": False}
    assert (train.FILL_DEFAULTS, train.GUIDED_DEFAULTS, train.NORM_DEFAULTS) == (
        {"fill_holes": False}, {"fill_guided": False, "fill_sigma": 10.0}, {"normalize": False})
    assert set(train.RESUME_ALL_DEFAULTS) | {"scale", "crop", "batch", "dtype"} == set(train.RESUME_ALL_KEYS)
