"""The one record of a training run's trajectory options (train.RunOptions) without a GPU: the checkpoint args of
every command line of tests/golden/train_args.json -- written by the commit BEFORE the record (tools/make_golden_train_args.py)
and never from the code under test -- come out key for key, value for value and type for type; the record fit builds from its
keyword arguments and its TrainSet equals the one the command line gives; a checkpoint from before every option resumes under
the plain command line only; and the public views of the table hold what they always held, written out here."""
import json
import os
import types

import pytest
import torch

from codon_amd import train
from codon_amd.prep import LrPrep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "train_args.json")) as fh:
    GOLDEN = json.load(fh)
RUNS = [(r["argv"], r["args"]) for r in GOLDEN["runs"]]
LEAST = ("", "--train-label l --mask-holes --min-valid 0.25", "--depth-bits 16 --depth-max 10000", "--degrade-holes",
         "--degrade-holes --fill-holes", "--train-lr-depth l --fill-holes --fill-guided --fill-sigma 6 --normalize",
         "--degrade-holes --sensor-noise 1.5 --sensor-dropout 0.05 --seed 9",
         "--lr-schedule cosine --steps 50 --warmup-steps 5 --lr-min 1e-6", "--lr-schedule cosine --steps 50 --lr-steps 200",
         "--clip-norm 1 --skip-nonfinite --ema 0.999", "--dtype f32 --crop 64 --batch 4")


def _parse(argv):
    return train.parse_args((GOLDEN["prefix"] + " " + argv).split())


def _typed(d):
    return {k: (type(v), v) for k, v in d.items()}


def test_the_fixture_is_the_parents():
    assert GOLDEN["prefix"] == "--scale 4 --train-depth d --train-color c"
    assert GOLDEN["provenance"]["commit"] == "8adf83f20308b25fce42b465508f923978b469e1"     # the commit before the record
    assert set(LEAST) <= {argv for argv, _ in RUNS}


@pytest.mark.parametrize("argv,want", RUNS, ids=[argv or "plain" for argv, _ in RUNS])
def test_run_args_are_the_parents(argv, want):
    got = train.run_args(_parse(argv))
    assert _typed(got) == _typed(want)
    assert _typed(json.loads(json.dumps(got))) == _typed(want)


@pytest.mark.parametrize("argv", [argv for argv, _ in RUNS], ids=[argv or "plain" for argv, _ in RUNS])
def test_two_constructors_one_record(argv):
    """What fit writes into a checkpoint (the record of its keyword arguments and its TrainSet) is what the command line that
    called it hands to load_resume (the record of the namespace)."""
    a = _parse(argv)
    # the TrainSet main builds for this command line: its pool is filled only where it holds real low-resolution maps
    built = a.prep if a.train_lr_depth is not None else LrPrep(normalize=a.normalize)
    ts = types.SimpleNamespace(has_label=a.train_label is not None, has_lr=a.train_lr_depth is not None,
                               depth_bits=a.depth_bits, depth_max=a.depth_max, prep=built)
    kw = train.fit_kwargs(a)
    of_a, of_fit = train.RunOptions.of_namespace(a), train.RunOptions.of_fit(ts, kw)
    assert of_a == of_fit
    assert _typed(of_a.args()) == _typed(of_fit.args())
    assert {**of_fit.args(), "lr": a.lr, "seed": a.seed} == train.run_args(a)
    assert {"lr": 5.0, "seed": 77, "other": "kept", **of_fit.args()}["other"] == "kept"
    # the names of fit's keyword arguments, and the options that are passed only when they are set
    assert ("ema_decay" in kw, "warmup" in kw, "ema" in kw, "warmup_steps" in kw) == (True, True, False, False)
    assert (kw["ema_decay"], kw["warmup"], kw["lr"]) == (a.ema, a.warmup_steps, a.lr)
    assert ("sensor" in kw) == ("--sensor" in argv) and kw.get("sensor") == train.sensor_of(a)
    assert {k: kw[k] for k in ("fill_holes", "fill_guided", "fill_sigma", "normalize") if k in kw} == a.prep.set_options()
    import inspect
    assert set(kw) <= {n for n, p in inspect.signature(train.fit).parameters.items() if p.kind is p.KEYWORD_ONLY}


def test_a_stand_in_that_disagrees_is_seen():
    """The second constructor reads the TrainSet, not the command line: another set gives another record."""
    a = _parse("--depth-bits 16 --depth-max 10000")
    ts = types.SimpleNamespace(has_label=False, has_lr=False, depth_bits=16, depth_max=10000, prep=LrPrep())
    same = train.RunOptions.of_fit(ts, train.fit_kwargs(a))
    assert same == train.RunOptions.of_namespace(a)
    for change in ({"has_label": True}, {"has_lr": True}, {"depth_max": 9999}, {"depth_bits": 8}):
        other = train.RunOptions.of_fit(types.SimpleNamespace(**{**vars(ts), **change}), train.fit_kwargs(a))
        assert other != same and other.args() != same.args(), change
    eight = train.RunOptions.of_fit(types.SimpleNamespace(**{**vars(ts), "depth_bits": 8}), train.fit_kwargs(a))
    assert not {"depth_bits", "depth_max"} & set(eight.args())               # an 8-bit run writes neither, whatever its depth_max
    with pytest.raises(Exception):
        same.crop = 1                                                        # frozen


OLD = {"scale": 4, "crop": 128, "batch": 16, "dtype": "bf16", "lr": 1e-4, "seed": 0}     # the args of the first checkpoints
REFUSED = {      # per command line of the matrix that sets a trajectory option: what load_resume says after "other arguments: "
    LEAST[1]: "mask_holes False != True, min_valid 0.0 != 0.25, train_label False != True",
    LEAST[2]: "depth_bits 8 != 16, depth_max 65535 != 10000",
    LEAST[3]: "degrade_holes False != True",
    LEAST[4]: "degrade_holes False != True, fill_holes False != True",
    LEAST[5]: "train_lr_depth False != True, fill_holes False != True, fill_guided False != True, fill_sigma 10.0 != 6.0, "
              "normalize False != True",
    LEAST[6]: "degrade_holes False != True, sensor_noise None != 1.5, sensor_noise_quad None != 0.0, sensor_dropout None != 0.05, "
              "sensor_edge_dropout None != 0.0, sensor_edge_threshold None != 0.0, sensor_seed None != 9",
    LEAST[7]: "lr_schedule 'constant' != 'cosine', warmup_steps 0 != 5, lr_min 0.0 != 1e-06, lr_steps None != 50",
    LEAST[8]: "lr_schedule 'constant' != 'cosine', lr_steps None != 200",
    LEAST[9]: "clip_norm None != 1.0, skip_nonfinite False != True, ema None != 0.999",
    LEAST[10]: "crop 128 != 64, batch 16 != 4, dtype 'bf16' != 'f32'",
}


def test_old_checkpoints(tmp_path):
    path = str(tmp_path / "old.pth")
    torch.save({"epoch": 3, "model": {}, "optimizer": {}, "rng": {}, "args": dict(OLD)}, path)
    assert train.load_resume(path, train.run_args(_parse("")))["epoch"] == 3
    assert set(REFUSED) == set(LEAST[1:])
    for argv, words in REFUSED.items():
        with pytest.raises(ValueError) as e:
            train.load_resume(path, train.run_args(_parse(argv)))
        assert str(e.value) == f"--resume {path}: the checkpoint was trained with other arguments: {words}", argv
    # and a checkpoint of each of those runs resumes under its own command line, and is refused under the plain one
    for argv in REFUSED:
        args = train.run_args(_parse(argv))
        torch.save({"epoch": 3, "model": {}, "optimizer": {}, "rng": {}, "args": args}, path)
        assert train.load_resume(path, args)["epoch"] == 3
        with pytest.raises(ValueError, match="the checkpoint was trained with other arguments: "):
            train.load_resume(path, train.run_args(_parse("")))
    torch.save({"epoch": 3, "model": {}}, path)
    with pytest.raises(ValueError, match="not a codon_amd.train checkpoint"):
        train.load_resume(path, dict(OLD))


def test_the_views_of_the_table():
    assert train.RESUME_KEYS == ("scale", "crop", "batch", "dtype", "clip_norm", "skip_nonfinite", "ema", "lr_schedule",
                                 "warmup_steps", "lr_min", "lr_steps", "mask_holes", "min_valid", "train_label")
    assert train.RESUME_DEFAULTS == {"clip_norm": None, "skip_nonfinite": False, "ema": None, "lr_schedule": "constant",
                                     "warmup_steps": 0, "lr_min": 0.0, "lr_steps": None, "mask_holes": False, "min_valid": 0.0,
                                     "train_label": False}
    assert train.DEPTH_DEFAULTS == {"depth_bits": 8, "depth_max": 65535}
    assert train.DEGRADE_DEFAULTS == {"degrade_holes": False}
    assert train.LR_DEFAULTS == {"train_lr_depth": False}
    assert train.SENSOR_DEFAULTS == {"sensor_noise": None, "sensor_noise_quad": None, "sensor_dropout": None,
                                     "sensor_edge_dropout": None, "sensor_edge_threshold": None, "sensor_seed": None}
    assert train.FILL_DEFAULTS == {"fill_holes": False}
    assert train.GUIDED_DEFAULTS == {"fill_guided": False, "fill_sigma": 10.0}
    assert train.NORM_DEFAULTS == {"normalize": False}
    assert train.RESUME_ALL_KEYS == train.RESUME_KEYS + (
        "depth_bits", "depth_max", "degrade_holes", "train_lr_depth", "sensor_noise", "sensor_noise_quad", "sensor_dropout",
        "sensor_edge_dropout", "sensor_edge_threshold", "sensor_seed", "fill_holes", "fill_guided", "fill_sigma", "normalize")
    assert train.RESUME_ALL_DEFAULTS == {
        "clip_norm": None, "skip_nonfinite": False, "ema": None, "lr_schedule": "constant", "warmup_steps": 0, "lr_min": 0.0,
        "lr_steps": None, "mask_holes": False, "min_valid": 0.0, "train_label": False, "depth_bits": 8, "depth_max": 65535,
        "degrade_holes": False, "train_lr_depth": False, "sensor_noise": None, "sensor_noise_quad": None, "sensor_dropout": None,
        "sensor_edge_dropout": None, "sensor_edge_threshold": None, "sensor_seed": None, "fill_holes": False, "fill_guided": False,
        "fill_sigma": 10.0, "normalize": False}
    assert list(train.RESUME_ALL_DEFAULTS) == list(train.RESUME_ALL_KEYS[4:])                 # and in the table's order
    for view in (train.RESUME_DEFAULTS, train.DEPTH_DEFAULTS, train.SENSOR_DEFAULTS, train.GUIDED_DEFAULTS):
        assert all(type(v) is type(train.RESUME_ALL_DEFAULTS[k]) for k, v in view.items())
    # the record's fields are the table's keys, the members standing for theirs
    import dataclasses
    fields = [f.name for f in dataclasses.fields(train.RunOptions)]
    assert fields == list(train.RESUME_ALL_KEYS[:18]) + ["sensor", "prep"]
