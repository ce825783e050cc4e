"""The options of a training run that change its trajectory: ONE table of the keys a checkpoint's args hold and
--resume compares, ONE record of a run's values for them, built from the command line or from what train.fit was called with,
and the one mapping from the command line to fit's keyword arguments.  The sensor model and prep.LrPrep (DESIGN
12.12) are the record's members and own their keys.  Nothing here needs a device; train.py imports every name."""
from __future__ import annotations

import dataclasses
import math

from .prep import LrPrep


@dataclasses.dataclass(frozen=True)
class SensorModel:
    """The sensor model of the synthetic degradation, applied to the low-resolution map between the two bicubics.
    noise, noise_quad, edge_threshold are in CODES of the data's own grid (255, or depth_max): the standard deviation of a
    valid pixel of value v is noise + noise_quad * v^2 codes (noise_quad: sensors whose noise grows with the square of the
    range; 0 for disparity-like data).  dropout is the probability that a valid pixel becomes a hole, edge_dropout the
    probability added where a 4-neighbour differs by more than edge_threshold codes; both need degrade_holes (a hole must be
    left out of the upsample, not smeared through it).  seed: 64 bits, the Philox key."""
    noise: float = 0.0
    noise_quad: float = 0.0
    dropout: float = 0.0
    edge_dropout: float = 0.0
    edge_threshold: float = 0.0
    seed: int = 0

    def __post_init__(self):
        for n in ("noise", "noise_quad", "edge_threshold"):
            v = getattr(self, n)
            if not (isinstance(v, (int, float)) and math.isfinite(v) and v >= 0):
                raise ValueError(f"SensorModel: {n} {v!r} must be finite and not negative")
        for n in ("dropout", "edge_dropout"):
            v = getattr(self, n)
            if not (isinstance(v, (int, float)) and 0.0 <= v <= 1.0):
                raise ValueError(f"SensorModel: {n} {v!r} must lie in [0, 1]")
        if self.dropout + self.edge_dropout > 1.0:
            raise ValueError(f"SensorModel: dropout {self.dropout} + edge_dropout {self.edge_dropout} exceeds 1")
        if not (isinstance(self.seed, int) and 0 <= self.seed < 1 << 64):
            raise ValueError(f"SensorModel: seed {self.seed!r} must be an integer of 64 bits, not negative")

    @property
    def drops(self) -> bool:
        return self.dropout > 0 or self.edge_dropout > 0

    def args(self) -> dict:
        """The checkpoint keys of SENSOR_DEFAULTS."""
        return {"sensor_noise": float(self.noise), "sensor_noise_quad": float(self.noise_quad),
                "sensor_dropout": float(self.dropout), "sensor_edge_dropout": float(self.edge_dropout),
                "sensor_edge_threshold": float(self.edge_threshold), "sensor_seed": int(self.seed)}


# THE table of the keys a checkpoint's args hold and --resume compares, in the order load_resume names them: per group, {key:
# what it compares as when a checkpoint's args lack it (one written before the option existed)} and when the group is written --
# ALWAYS, or WHEN_SET: by a run that sets one of its keys to something else than that default ONLY, so that a run without the
# option keeps exactly the keys checkpoints always had.  A new option is a row here and a field of RunOptions.
ALWAYS, WHEN_SET = "always", "when set"
RESUME_TABLE = (
    (dict.fromkeys(("scale", "crop", "batch", "dtype")), ALWAYS),          # in every checkpoint: no default to compare as
    ({"clip_norm": None, "skip_nonfinite": False, "ema": None, "lr_schedule": "constant", "warmup_steps": 0, "lr_min": 0.0,
      "lr_steps": None, "mask_holes": False, "min_valid": 0.0, "train_label": False}, ALWAYS),
    ({"depth_bits": 8, "depth_max": 65535}, WHEN_SET),                     # a 16-bit run
    ({"degrade_holes": False}, WHEN_SET),
    ({"train_lr_depth": False}, WHEN_SET),
    (dict.fromkeys(SensorModel().args()), WHEN_SET),                       # a run with a model; None: no model
    (LrPrep.defaults("fill_holes"), WHEN_SET),
    (LrPrep.defaults("fill_guided", "fill_sigma"), WHEN_SET),
    (LrPrep.defaults("normalize"), WHEN_SET),
)
# the table's views: its groups by name, and what load_resume compares
_always, _when_set = ([d for d, written in RESUME_TABLE if written is w] for w in (ALWAYS, WHEN_SET))
_REQUIRED, RESUME_DEFAULTS = _always
DEPTH_DEFAULTS, DEGRADE_DEFAULTS, LR_DEFAULTS, SENSOR_DEFAULTS, FILL_DEFAULTS, GUIDED_DEFAULTS, NORM_DEFAULTS = _when_set
RESUME_KEYS = tuple(_REQUIRED) + tuple(RESUME_DEFAULTS)
RESUME_ALL_KEYS = tuple(k for d, _ in RESUME_TABLE for k in d)
RESUME_ALL_DEFAULTS = {k: v for d, _ in RESUME_TABLE[1:] for k, v in d.items()}


def _from(**where):
    return dataclasses.field(metadata=where)


@dataclasses.dataclass(frozen=True)
class RunOptions:
    """The trajectory options of ONE run: a field per key of RESUME_TABLE, the sensor model and the preparation as members
    standing for their keys.  args() is what a checkpoint's args hold of them.  A field says where fit finds its value when that
    is not a keyword argument of its own name: fit= another name, trainset= an attribute of the TrainSet."""
    scale: int
    crop: int
    batch: int
    dtype: str
    clip_norm: float
    skip_nonfinite: bool
    ema: float = _from(fit="ema_decay")
    lr_schedule: str
    warmup_steps: int = _from(fit="warmup")
    lr_min: float
    lr_steps: int                   # the length of the cosine curve, resolved (parse_args, fit); None under another schedule
    mask_holes: bool
    min_valid: float
    train_label: bool = _from(trainset="has_label")
    depth_bits: int = _from(trainset="depth_bits")
    depth_max: int = _from(trainset="depth_max")        # the default with 8 bits, where it means nothing
    degrade_holes: bool
    train_lr_depth: bool = _from(trainset="has_lr")
    sensor: SensorModel             # or None
    prep: LrPrep

    def __post_init__(self):
        """Equal runs give equal records: a value takes the type of its default in the table where that is a bool, an int or a
        float, and an option that means nothing without another one takes its default."""
        def put(**values):
            for n, v in values.items():
                object.__setattr__(self, n, v)
        for f in _OWN:
            kind = type(RESUME_ALL_DEFAULTS.get(f.name))
            if kind in (bool, int, float):
                put(**{f.name: kind(getattr(self, f.name))})
        if self.lr_schedule != "cosine":
            put(lr_steps=None)
        if self.depth_bits != 16:
            put(**DEPTH_DEFAULTS)

    @classmethod
    def of_namespace(cls, a) -> "RunOptions":
        """The record of a command line (train.parse_args' namespace); a directory option counts as whether it was given."""
        own = {f.name: getattr(a, f.name) for f in _OWN}
        return cls(**dict(own, train_label=a.train_label is not None, train_lr_depth=a.train_lr_depth is not None),
                   sensor=sensor_of(a), prep=a.prep)

    @classmethod
    def of_fit(cls, trainset, kw: dict) -> "RunOptions":
        """The record of a call of train.fit: kw holds fit's keyword arguments under their names there (fit's own locals, or
        fit_kwargs(a); sensor and the preparation's may be missing, as in a call without them), lr_steps resolved; `trainset`
        is read for has_label, has_lr, depth_bits and depth_max only.  The preparation's values are checked under fit's name."""
        own = {f.name: getattr(trainset, f.metadata["trainset"]) if "trainset" in f.metadata else kw[f.metadata.get("fit", f.name)]
               for f in _OWN}
        prep = {f.name: kw[f.name] for f in dataclasses.fields(LrPrep) if f.name in kw}
        return cls(**own, sensor=kw.get("sensor"), prep=LrPrep.checked("fit", **prep))

    def args(self) -> dict:
        """The checkpoint's args: the table's keys under its written-when-set rule, stated here and nowhere else."""
        now = {f.name: getattr(self, f.name) for f in _OWN}
        now.update(SENSOR_DEFAULTS if self.sensor is None else self.sensor.args(), **dataclasses.asdict(self.prep))
        return {k: now[k] for d, written in RESUME_TABLE if written is ALWAYS or any(now[k] != v for k, v in d.items()) for k in d}


_OWN = dataclasses.fields(RunOptions)[:-2]              # the fields that are keys themselves


# ---- from the command line ------------------------------------------------------------------------------------------------------

def sensor_of(a):
    """The SensorModel the command line asks for, or None when it names no --sensor option."""
    f = {n: getattr(a, "sensor_" + n) for n in ("noise", "noise_quad", "dropout", "edge_dropout", "edge_threshold")}
    if all(v is None for v in f.values()):
        return None
    return SensorModel(seed=a.seed, **{n: 0.0 if v is None else v for n, v in f.items()})


def run_args(a) -> dict:
    """What --resume compares and a checkpoint's args start from: the record's keys, with lr and seed beside them."""
    return {**RunOptions.of_namespace(a).args(), "lr": a.lr, "seed": a.seed}


def fit_kwargs(a) -> dict:
    """The keyword arguments of train.fit that the command line decides, under fit's names for them.  A sensor model and the
    preparation's options are passed when they are set only: without them fit is called as ever."""
    o = RunOptions.of_namespace(a)
    kw = {f.metadata.get("fit", f.name): getattr(o, f.name) for f in _OWN if "trainset" not in f.metadata}
    return {**kw, "lr": a.lr, "log_every": a.log_every, **({"sensor": o.sensor} if o.sensor is not None else {}),
            **o.prep.set_options()}
